"""The ARP / ICMPv6 responders — gf_respond (tail_handle_arp, tail_icmp6_handle_ns,
tail_icmp6_send_echo_reply, tail_icmp6_send_time_exceeded) and gf_respond_calls.

The CPU oracle cannot express the responders.  The checks rest on:

 1. known answers (tests/golden/respond_kats.json): every expected reply built field by field,
    its ICMPv6 checksum recomputed in full over the pseudo header and the message;
 2. tests/respond_model.py, a per-frame restatement from the reference text, which reproduces
    the known answers and is itself checked by a from-scratch checksum verification of every
    reply it produces over a fuzz batch;
 3. on the device: byte equality with both, over strides 122 / 128 / 256, block boundaries,
    poisoned snap_out rows, the drop records of an event ring, and end to end behind
    gf_lxc_egress_classify and gf_pipeline_classify, whose own outputs must not change.
"""
import ctypes as C
import errno
import json
import os
import struct

import numpy as np
import pytest

from cilium_amd import synth
from cilium_amd import _lib
from cilium_amd._lib import lib, gf_frames, gf_respond_cfg, gf_respond_batch, gf_event_ring
from tests import respond_model as M

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FUZZ_SEED, FUZZ_N = 11, 20000


def _kats():
    with open(os.path.join(GOLDEN, "respond_kats.json")) as f:
        return json.load(f)["cases"]


def _kat_arrays(cases):
    S = 128
    frames = np.stack([np.frombuffer(bytes.fromhex(c["frame"]), np.uint8) for c in cases]).copy()
    lens = np.array([c["len"] for c in cases], np.uint32)
    calls = np.array([c["call"] for c in cases], np.uint8)
    want = np.zeros(len(cases), M.RESP_OUT)
    rows = np.full((len(cases), S), 0xA5, np.uint8)          # unwritten rows keep the poison
    for k, c in enumerate(cases):
        for name, v in c["expect"].items():
            want[k][name] = v
        if c["row"] is not None:
            rows[k] = np.frombuffer(bytes.fromhex(c["row"]), np.uint8)
    return frames, lens, calls, want, rows


def _kat_groups():
    groups = {}
    for c in _kats():
        groups.setdefault((c["flags"], c["max_len"], c["lxc_id"] is not None), []).append(c)
    return groups


_fuzz_cache = {}


def fuzz_batch(stride, with_lxc):
    """One fuzz batch and the model's answer per (stride, with_lxc), computed once."""
    key = (stride, with_lxc)
    if key not in _fuzz_cache:
        frames, lens, calls, lxc, fh = M.fuzz(FUZZ_SEED + stride + with_lxc, FUZZ_N, stride, with_lxc)
        init = np.full_like(frames, 0xA5)
        rec, snap, ev = M.respond(M.default_cfg(), frames, lens, calls, lxc, fh, init)
        _fuzz_cache[key] = (frames, lens, calls, lxc, fh, rec, snap, ev)
    return _fuzz_cache[key]


# ---------------------------------------------------------------- CPU
def test_kat_file_covers_the_listed_cases():
    names = {c["name"] for c in _kats()}
    assert {"arp_hit_bcast", "arp_hit_unicast_lxc", "arp_wrong_tip", "arp_wrong_op", "arp_len41", "ns_hit",
            "ns_unknown_target_drop", "ns_unknown_target_to_stack", "ns_len77", "ns_len85", "echo_hit", "te_udp", "te_tcp",
            "te_icmp6_lxc", "te_unknown_proto", "te_udp_short", "te_tcp_short", "te_udp_padding", "te_over_max_len",
            "te_under_54", "call_7", "empty_lxc_slot"} <= names
    for c in _kats():
        if c["expect"]["action"] == M.TC_REDIRECT and c["call"] != M.CALL_ARP:
            assert M.icmp6_checksum_ok(bytes.fromhex(c["row"])), c["name"]


def test_model_reproduces_every_kat():
    for (flags, max_len, with_lxc), cases in _kat_groups().items():
        frames, lens, calls, want, rows = _kat_arrays(cases)
        lxc = np.array([c["lxc_id"] for c in cases], np.uint16) if with_lxc else None
        rec, snap, _ = M.respond(M.default_cfg(flags, max_len), frames, lens, calls, lxc, None, np.full_like(frames, 0xA5))
        for k, c in enumerate(cases):
            assert rec[k] == want[k], (c["name"], rec[k], want[k])
            assert np.array_equal(snap[k], rows[k]), (c["name"], np.nonzero(snap[k] != rows[k])[0])


@pytest.mark.parametrize("with_lxc", [True, False])
def test_model_replies_verify_from_scratch(with_lxc):
    """Not the model's arithmetic: every REDIRECT ICMPv6 reply of a fully captured frame whose request
    checksum was valid (or which is a time-exceeded reply, whose checksum is computed anew) carries a
    checksum that a from-scratch sum over pseudo header and message verifies; every ARP reply names
    the gateway as sender and the requester as target."""
    stride = 128
    frames, lens, calls, lxc, fh, rec, snap, ev = fuzz_batch(stride, with_lxc)
    checked = {M.CALL_NS: 0, M.CALL_ECHO: 0, M.CALL_TE: 0}
    arps = 0
    for i in np.nonzero(rec["action"] == M.TC_REDIRECT)[0]:
        c, row = int(calls[i]), bytes(snap[i])
        mac = M.PROGS[int(lxc[i])][0] if with_lxc else M.NODE_MAC
        if c == M.CALL_ARP:
            rq = bytes(frames[i])
            assert row[22:28] == mac and row[28:32] == M.GATEWAY            # ar_sha, ar_sip
            assert row[32:38] == rq[6:12] and row[38:42] == rq[28:32]       # ar_tha, ar_tip
            assert row[0:6] == rq[6:12] and row[6:12] == mac and row[20:22] == b"\x00\x02"
            arps += 1
            continue
        assert row[22:38] == M.ROUTER and row[38:54] == bytes(frames[i, 22:38]) and row[6:12] == mac
        if rec[i]["len"] > stride:
            continue
        if c != M.CALL_TE and (lens[i] > stride or not M.icmp6_checksum_ok(bytes(frames[i]))):
            continue
        assert M.icmp6_checksum_ok(row), (i, c)
        checked[c] += 1
    assert arps > 500 and all(v > 300 for v in checked.values()), (arps, checked)


@pytest.mark.parametrize("stride,with_lxc", [(128, True), (128, False), (122, True), (256, False)])
def test_fuzz_batches_are_not_thin(stride, with_lxc):
    frames, lens, calls, lxc, fh, rec, snap, ev = fuzz_batch(stride, with_lxc)
    n = len(calls)
    for c in range(5):
        assert (calls == c).sum() >= 0.10 * n, c
    assert (rec["action"] == M.TC_REDIRECT).any() and ((rec["action"] == M.TC_OK) & (calls != 0)).any()
    for reason in (134, 140, 141, 142, 150):
        assert ((rec["action"] == M.TC_SHOT) & (rec["reason"] == reason)).any(), reason
    cls = {}
    for c, a, r in zip(calls.tolist(), rec["action"].tolist(), rec["reason"].tolist()):
        cls[(c, a, r)] = cls.get((c, a, r), 0) + 1
    assert max(cls.values()) <= 0.60 * n
    assert len(ev) == (rec["action"] == M.TC_SHOT).sum()


def _load(flags=0, max_len=0, array=0):
    cfg = gf_respond_cfg(array, flags, max_len)
    return lib.gf_respond_load(C.byref(cfg))


def test_refusals_without_a_device():
    """Every refusal precedes any launch, so none of these needs a GPU (the pointers are never
    dereferenced)."""
    assert lib.gf_respond_load(None) == -errno.EFAULT
    assert _load(flags=2) == -errno.EINVAL
    assert _load(array=999999) == -errno.EBADF
    h = _load()
    assert h > 0
    P = 0x1000                                           # a non-NULL stand-in
    ok = lambda n=4, stride=128, snap=P, ln=P, call=P: gf_respond_batch(gf_frames(n, stride, snap, ln), call, None, None)
    b = ok()
    assert lib.gf_respond(999999, C.byref(b), P, 2 * P, None) == -errno.EBADF
    pa = lib.gf_policy_array_create()
    assert lib.gf_respond(pa, C.byref(b), P, 2 * P, None) == -errno.EBADF       # a handle, but no responder
    assert lib.gf_respond(h, None, P, 2 * P, None) == -errno.EFAULT
    b0 = ok(n=0, snap=None, ln=None, call=None)
    assert lib.gf_respond(h, C.byref(b0), None, None, None) == 0
    for bad in (ok(snap=None), ok(ln=None), ok(call=None)):
        assert lib.gf_respond(h, C.byref(bad), P, 2 * P, None) == -errno.EFAULT
    assert lib.gf_respond(h, C.byref(b), None, 2 * P, None) == -errno.EFAULT
    assert lib.gf_respond(h, C.byref(b), P, None, None) == -errno.EFAULT
    for stride in (0, 64, 121, 257, 512):
        bs = ok(stride=stride)
        assert lib.gf_respond(h, C.byref(bs), P, 2 * P, None) == -errno.EINVAL, stride
    assert lib.gf_respond(h, C.byref(b), P, P, None) == -errno.EINVAL           # snap_out == frames.snap
    big = ok(n=(1 << 30) + 1)
    assert lib.gf_respond(h, C.byref(big), P, 2 * P, None) == -errno.E2BIG
    fr = gf_frames(4, 128, P, P)
    assert lib.gf_respond_calls(None, P, 1, P, None) == -errno.EFAULT
    assert lib.gf_respond_calls(C.byref(fr), P, 0, P, None) == -errno.EINVAL
    assert lib.gf_respond_calls(C.byref(fr), P, 3, P, None) == -errno.EINVAL
    assert lib.gf_respond_calls(C.byref(fr), None, 1, P, None) == -errno.EFAULT
    assert lib.gf_respond_calls(C.byref(fr), P, 2, None, None) == -errno.EFAULT
    fr0 = gf_frames(0, 128, None, None)
    assert lib.gf_respond_calls(C.byref(fr0), None, 2, None, None) == 0
    frb = gf_frames((1 << 30) + 1, 128, P, P)
    assert lib.gf_respond_calls(C.byref(frb), P, 2, P, None) == -errno.E2BIG
    lib.gf_obj_close(h)
    lib.gf_obj_close(pa)


def test_binding_constants_match_the_header():
    txt = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "gpuflow.h")).read()
    for name in ("GF_CALL_NONE", "GF_CALL_ARP", "GF_CALL_ICMP6_NS", "GF_CALL_ICMP6_ECHO_REPLY", "GF_CALL_ICMP6_TIME_EXCEEDED",
                 "GF_DROP_UNKNOWN_TARGET", "GF_REC_EGRESS", "GF_REC_PIPELINE"):
        import re
        m = re.search(r"#define\s+%s\s+(\d+)" % name, txt)
        assert m and int(m.group(1)) == getattr(_lib, name), name
    assert C.sizeof(gf_respond_cfg) == 12 and C.sizeof(gf_respond_batch) == C.sizeof(gf_frames) + 24


# ---------------------------------------------------------------- GPU
def _scenario():
    """The node and endpoint programs of respond_model.default_cfg (no maps: the responders read none)."""
    sc = synth.Scenario("respond", host_ifindex=3)
    sc.node = {"ipv4_gateway": struct.unpack("<I", M.GATEWAY)[0], "router_ip6": M.ROUTER, "node_mac": M.NODE_MAC}
    for lid, (mac, _) in sorted(M.PROGS.items()):
        sc.lxc.append({"lxc_id": lid, "seclabel": 500 + lid, "flags": 0, "l4": [], "node_mac": mac})
    return sc


def _dev(a, dt=None):
    import torch
    a = np.ascontiguousarray(a if dt is None else a.astype(dt))
    signed = {np.dtype(np.uint32): np.int32, np.dtype(np.uint16): np.int16, np.dtype(np.uint8): np.uint8}
    return torch.from_numpy(a.view(signed[a.dtype])).cuda()


def _gpu_respond(dp, frames, lens, calls, lxc=None, fh=None, flags=0, max_len=0, poison=0xA5):
    import torch
    snap = torch.full(frames.shape, poison, dtype=torch.uint8, device="cuda")
    out, snap = dp.respond(_dev(frames), _dev(lens, np.uint32), _dev(calls, np.uint8), None if lxc is None else _dev(lxc, np.uint16),
                           None if fh is None else _dev(fh, np.uint32), snap_out=snap, flags=flags, max_len=max_len)
    torch.cuda.synchronize()
    return out.cpu().numpy().view(M.RESP_OUT).reshape(-1), snap.cpu().numpy()


def _assert_same(got, gsnap, rec, snap, what):
    bad = np.nonzero(got != rec)[0]
    assert len(bad) == 0, f"{what}: {len(bad)} records differ, first {bad[0]}: {got[bad[0]]} vs {rec[bad[0]]}"
    bad = np.nonzero((gsnap != snap).any(axis=1))[0]
    assert len(bad) == 0, (f"{what}: {len(bad)} rows differ, first {bad[0]} (call {rec[bad[0]]['call']}) at bytes "
                           f"{np.nonzero(gsnap[bad[0]] != snap[bad[0]])[0][:12]}")


@pytest.fixture(scope="module")
def dp():
    from cilium_amd.datapath import Datapath
    d = Datapath(_scenario(), pin_prefix=None)
    yield d
    d.close()


@pytest.mark.gpu
def test_gpu_kats(dp):
    """Records and snap_out rows byte-equal to the golden file; rows the call does not write keep the
    caller's bytes."""
    for (flags, max_len, with_lxc), cases in _kat_groups().items():
        frames, lens, calls, want, rows = _kat_arrays(cases)
        lxc = np.array([c["lxc_id"] for c in cases], np.uint16) if with_lxc else None
        got, gsnap = _gpu_respond(dp, frames, lens, calls, lxc, flags=flags, max_len=max_len)
        for k, c in enumerate(cases):
            assert got[k] == want[k], (c["name"], got[k], want[k])
            assert np.array_equal(gsnap[k], rows[k]), (c["name"], np.nonzero(gsnap[k] != rows[k])[0])


@pytest.mark.gpu
@pytest.mark.parametrize("stride,with_lxc,events", [(128, True, True), (128, False, False), (122, True, False),
                                                    (256, False, False), (256, True, False)])
def test_gpu_fuzz_parity(dp, stride, with_lxc, events):
    """~20k frames against the model: records, reply rows, the 0xA5 poison of every row without a call
    (or with a missed tail call), and with an event ring the drop records."""
    import torch
    frames, lens, calls, lxc, fh, rec, snap, ev = fuzz_batch(stride, with_lxc)
    if events:
        cap = len(ev) + 64
        recs = torch.zeros((cap, 160), dtype=torch.uint8, device="cuda")
        cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
        ring = gf_event_ring(recs.data_ptr(), cap, cnt.data_ptr())
        assert lib.gf_set_event_ring(C.byref(ring)) == 0
    try:
        got, gsnap = _gpu_respond(dp, frames, lens, calls, lxc, fh)
        _assert_same(got, gsnap, rec, snap, f"stride {stride}")
        quiet = (calls == 0) | (rec["reason"] == 140)
        assert quiet.sum() > 3000 and (gsnap[quiet] == 0xA5).all()
        if events:
            n = int(cnt.item())
            assert n == len(ev) > 1000
            g = recs[:n].cpu().numpy()
            e = np.frombuffer(b"".join(ev), np.uint8).reshape(n, 160)
            bad = np.nonzero((g != e).any(axis=1))[0]
            assert len(bad) == 0, f"{len(bad)} drop records differ, first {bad[:1]}: {g[bad[0]][:32]} vs {e[bad[0]][:32]}"
    finally:
        if events:
            lib.gf_set_event_ring(None)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257])
def test_gpu_block_boundaries(dp, n):
    frames, lens, calls, lxc, fh, rec, snap, ev = fuzz_batch(128, True)
    if n == 0:
        import torch
        e = torch.empty((0, 128), dtype=torch.uint8, device="cuda")
        out, _ = dp.respond(e, torch.empty(0, dtype=torch.int32, device="cuda"), torch.empty(0, dtype=torch.uint8, device="cuda"))
        assert out.shape[0] == 0
        return
    for start in (0, 1000):                              # two windows of the batch, so the mix differs
        s = slice(start, start + n)
        got, gsnap = _gpu_respond(dp, frames[s], lens[s], calls[s], lxc[s], fh[s])
        _assert_same(got, gsnap, rec[s], snap[s], f"n {n} at {start}")


@pytest.mark.gpu
@pytest.mark.parametrize("stride", [128, 250])
def test_gpu_all_calls_zero_touches_no_row(dp, stride):
    n = 3000
    rng = np.random.default_rng(5)
    frames = rng.integers(0, 256, (n, stride), dtype=np.uint8)
    lens = rng.integers(0, 1600, n).astype(np.uint32)
    got, gsnap = _gpu_respond(dp, frames, lens, np.zeros(n, np.uint8))
    want = np.zeros(n, M.RESP_OUT)
    want["len"] = lens
    assert np.array_equal(got, want)
    assert (gsnap == 0xA5).all()


def _model_cfg(sc):
    nd = sc.node or {}
    progs = {e["lxc_id"]: (bytes(e.get("node_mac", bytes(6))), e["lxc_id"]) for e in sc.lxc}
    return M.Cfg(struct.pack("<I", nd.get("ipv4_gateway", 0)), nd.get("router_ip6", bytes(16)), nd.get("node_mac", bytes(6)), progs)


def _calls_of(kind, frames, lens, rec):
    if kind == _lib.GF_REC_PIPELINE:
        return np.where(rec["flags"] & 0x20, 4, 0).astype(np.uint8)
    ef = rec["eg_flags"]
    b54 = np.where(lens > 54, frames[:, 54], 0)
    return np.where(ef & 0x800, 1, np.where(ef & 0x4000, np.where(b54 == 135, 2, 3), np.where(ef & 0x2000, 4, 0))).astype(np.uint8)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["egress", "pipeline"])
def test_gpu_end_to_end(kind):
    """classify -> respond_after over the existing fuzz scenarios (which hold ARP, NS, echo-to-router and
    hop-limit-expired frames): the derived call column, the records and the reply frames equal the model
    fed the same frames, and the classify call's own records and frames are byte-identical to a run
    without the responder call."""
    import torch
    from cilium_amd.datapath import Datapath, DeviceBatch, EG_OUT, PIPE_OUT
    eg = kind == "egress"
    mk = (lambda: synth.egress_fuzz(seed=5, n_packets=6000, n_batches=1)) if eg else \
        (lambda: synth.pipeline_fuzz(seed=3, n_packets=6000, n_batches=1))
    runs = []
    for with_responder in (False, True):
        sc = mk()
        d = Datapath(sc, pin_prefix=None)
        pk = sc.batches[0]
        b = DeviceBatch(pk, parse=False)
        if eg:
            out, snap = d.egress(b, sc.now)
        else:
            out, _, snap = d.pipeline(b, sc.now)
        extra = None
        if with_responder:
            call, rout, reply = d.respond_after(_lib.GF_REC_EGRESS if eg else _lib.GF_REC_PIPELINE, b, out, snap)
            torch.cuda.synchronize()
            extra = (call.cpu().numpy(), rout.cpu().numpy().view(M.RESP_OUT).reshape(-1), reply.cpu().numpy())
        torch.cuda.synchronize()
        runs.append((out.cpu().numpy().copy(), snap.cpu().numpy().copy(), extra, sc, pk))
        d.close()
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])
    rec8, snap, (call, rout, reply), sc, pk = runs[1]
    rec = rec8.view(EG_OUT if eg else PIPE_OUT).reshape(-1)
    want_call = _calls_of(_lib.GF_REC_EGRESS if eg else _lib.GF_REC_PIPELINE, pk.frames, pk.lens, rec)
    assert np.array_equal(call, want_call)
    for c in ((1, 2, 3, 4) if eg else (4,)):
        assert (call == c).any(), c
    frames = np.where((call == 4)[:, None], snap, pk.frames)
    mrec, msnap, _ = M.respond(_model_cfg(sc), frames, pk.lens, call, pk.lxc_id if eg else None, None, None)
    assert np.array_equal(rout, mrec)
    live = call != 0
    assert np.array_equal(reply[live], msnap[live])
    assert (mrec["action"][live] == M.TC_REDIRECT).sum() > (20 if eg else 3)


@pytest.mark.gpu
def test_gpu_refusals(dp):
    """With real device buffers: the refusals leave out and snap_out untouched."""
    import torch
    frames, lens, calls, lxc, fh, rec, snap, ev = fuzz_batch(128, True)
    n = 100
    f, ln, c = _dev(frames[:n]), _dev(lens[:n], np.uint32), _dev(calls[:n], np.uint8)
    out = torch.full((n, 8), 0x5A, dtype=torch.uint8, device="cuda")
    so = torch.full((n, 128), 0x5A, dtype=torch.uint8, device="cuda")
    h = dp.responder()
    mkb = lambda stride=128, call=c.data_ptr(): gf_respond_batch(gf_frames(n, stride, f.data_ptr(), ln.data_ptr()), call, None, None)
    b = mkb()
    assert lib.gf_respond(dp.policy_array, C.byref(b), out.data_ptr(), so.data_ptr(), None) == -errno.EBADF
    assert lib.gf_respond(h, C.byref(mkb(call=None)), out.data_ptr(), so.data_ptr(), None) == -errno.EFAULT
    assert lib.gf_respond(h, C.byref(b), out.data_ptr(), None, None) == -errno.EFAULT
    assert lib.gf_respond(h, C.byref(mkb(stride=64)), out.data_ptr(), so.data_ptr(), None) == -errno.EINVAL
    assert lib.gf_respond(h, C.byref(b), out.data_ptr(), f.data_ptr(), None) == -errno.EINVAL
    torch.cuda.synchronize()
    assert (out == 0x5A).all() and (so == 0x5A).all()
    # a responder without a policy array: every slot is empty
    cfg = gf_respond_cfg(0, 0, 0)
    h0 = lib.gf_respond_load(C.byref(cfg))
    lb = gf_respond_batch(gf_frames(n, 128, f.data_ptr(), ln.data_ptr()), c.data_ptr(), _dev(lxc[:n], np.uint16).data_ptr(), None)
    assert lib.gf_respond(h0, C.byref(lb), out.data_ptr(), so.data_ptr(), None) == 0
    torch.cuda.synchronize()
    got = out.cpu().numpy().view(M.RESP_OUT).reshape(-1)
    live = calls[:n] != 0
    assert (got["reason"][live] == 140).all() and (got["action"][~live] == 0).all() and (so == 0x5A).all()
    lib.gf_obj_close(h0)
