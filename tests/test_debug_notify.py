"""Debug notifications (bpf/lib/dbg.h, the endpoint's Debug option): the hand-derived
known answers of tests/golden/dbg_kats.json against the Python restatement
(tests/dbg_model.py), the model anchored on the C oracle (verdicts and final CT
contents), and cilium_amd.monitor decoding hand-built records of the four types.
CPU only; the GPU side is tests/test_gpu_debug_notify.py."""
import ipaddress
import json
import os
import struct

import numpy as np

from cilium_amd import monitor as MON
from cilium_amd import synth
from cilium_amd.synth import Packets
from oracle.scenario import OracleDP
from tests import dbg_model as M

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NOW, IFINDEX, HOST_IFINDEX = 5000, 11, 3
LXC_DEBUG = synth.LXC_DEBUG
SRC4, SRC6 = synth.ip4("10.2.0.5"), ipaddress.IPv6Address("2001:db8::5").packed
PROTO = {"tcp": synth.TCP, "udp": synth.UDP, "icmp": synth.ICMP, "icmpv6": synth.ICMPV6, "gre": 47}
BASE_FLAGS = synth.LXC_PRODUCTION | synth.LXC_TRACE_NOTIFY


def kats():
    with open(os.path.join(GOLDEN, "dbg_kats.json")) as f:
        return json.load(f)["cases"]


def ep_addr(k):
    return synth.ip4("10.1.0.1") + k, ipaddress.IPv6Address(int(ipaddress.IPv6Address("f00d::1")) + (k << 32)).packed


def scenario(n_ep=1, debug=(0,), ct=None, prefill=(), local=False, px_max=4096):
    """n_ep endpoints (LXC_ID 100 + k, SECLABEL 300 + k, 10.1.0.1 + k / f00d::k:0:1) with the KAT policy;
    those listed in `debug` carry the Debug option.  prefill: CT entries of endpoint 0 as
    ct_create of the other direction would have left them ("forward": of the packets' own
    direction; "ct_flags": the entry's flag bits, seen_non_syn by default)."""
    sc = synth.Scenario("dbg", now=NOW, host_ifindex=HOST_IFINDEX)
    sc.add_map(synth.MapSpec("cilium_proxy4", synth.HASH, 10, 16, px_max, 0))
    sc.add_map(synth.MapSpec("cilium_proxy6", synth.HASH, 22, 28, px_max, 0))
    sc.node = {"proxy4": "cilium_proxy4", "proxy6": "cilium_proxy6", "ipv4_gateway": 0xfffff50a,
               "host_ip6": bytes([0xbe, 0xef] + [0] * 13 + [1]), "host_mac": bytes([0xce, 0x72, 0xa7, 0x03, 0x88, 0x56]),
               "node_mac": bytes([0xde, 0xad, 0xbe, 0xef, 0xc0, 0xde])}
    ct = ct or {}
    ctype = synth.HASH if ct.get("type") == "hash" else synth.LRU_HASH
    e4, e6 = ep_addr(0)
    k4, v4, k6, v6 = [], [], [], []
    for p in prefill:
        nh = PROTO[p["proto"]]
        val = synth.ct_vals(1, p["lifetime"], p.get("ct_flags", 16), 0, 300)
        if p.get("family") == 6:
            k6.append(synth.pack_rows(np.frombuffer(e6, np.uint8)[None], np.frombuffer(SRC6, np.uint8)[None],
                                      synth.le_bytes(synth.raw16([p["sport"]]), "<u2"),
                                      synth.le_bytes(synth.raw16([p["dport"]]), "<u2"), np.full((1, 1), nh, np.uint8),
                                      np.full((1, 1), p.get("flags", 0), np.uint8), np.zeros((1, 2), np.uint8)))
            v6.append(val)
        elif p.get("forward"):                                    # as an earlier packet of the same direction left it
            k4.append(synth.ct4_keys([SRC4], [e4], synth.raw16([p["dport"]]), synth.raw16([p["sport"]]), [nh], [1]))
            v4.append(val)
        else:
            k4.append(synth.ct4_keys([e4], [SRC4], synth.raw16([p["sport"]]), synth.raw16([p["dport"]]), [nh],
                                     [p.get("flags", 0)]))
            v4.append(val)
    cat = lambda a: np.concatenate(a) if a else None
    names4 = [f"ct4_{k}" if local else "ct4" for k in range(n_ep)]
    names6 = [f"ct6_{k}" if local else "ct6" for k in range(n_ep)]
    for j, n in enumerate(dict.fromkeys(names4)):
        sc.add_map(synth.MapSpec(n, ctype, 14, 48, ct.get("max_entries", 4096), 0, cat(k4) if j == 0 else None,
                                 cat(v4) if j == 0 else None))
    for j, n in enumerate(dict.fromkeys(names6)):
        sc.add_map(synth.MapSpec(n, ctype, 40, 48, ct.get("max_entries", 4096), 0, cat(k6) if j == 0 else None,
                                 cat(v6) if j == 0 else None))
    for k in range(n_ep):
        pk_ = synth.policy_keys([1000, 1000, 1000, 2000], [80, 8080, 53, 0], [synth.TCP, synth.TCP, synth.UDP, 0])
        sc.add_map(synth.MapSpec(f"pol{k}", synth.HASH, 8, 24, 1024, 0, pk_, synth.policy_vals([0, 15001, 0, 0])))
        sc.lxc.append({"lxc_id": 100 + k, "seclabel": 300 + k, "policy": f"pol{k}", "ct4": names4[k], "ct6": names6[k],
                       "flags": BASE_FLAGS | (LXC_DEBUG if k in debug else 0), "l4": []})
    return sc


def packets(specs):
    """specs: dicts {ep, family, id, proto, sport, dport, tcp_flags, icmp_type, tc_index, l4_keep, src}."""
    fr, ln, sid, lid, tci, fh = [], [], [], [], [], []
    for j, p in enumerate(specs):
        k = p.get("ep", 0)
        e4, e6 = ep_addr(k)
        nh = PROTO[p["proto"]]
        sport, dport = p.get("sport", 40000), p.get("dport", 0)
        if p.get("family") == 6:
            src = bytearray(SRC6)
            src[8] = p.get("src", 0)
            nh6 = synth.ICMPV6 if nh == synth.ICMP else nh
            f, l_ = synth.frames_v6(1, 128, np.frombuffer(bytes(src), np.uint8)[None], np.frombuffer(e6, np.uint8)[None], nh6,
                                    sport, dport, p.get("tcp_flags", 0), p.get("icmp_type", 0))
            l4 = 54
        else:
            f, l_ = synth.frames_v4(1, 128, SRC4 + (p.get("src", 0) << 8), e4, nh, sport, dport, p.get("tcp_flags", 0),
                                    p.get("icmp_type", 0))
            l4 = 34
        if "l4_keep" in p:
            l_ = np.array([l4 + p["l4_keep"]], np.uint32)
        fr.append(f); ln.append(l_); sid.append(p["id"]); lid.append(100 + k); tci.append(p.get("tc_index", 0))
        fh.append(0xabc00000 + j)
    n = len(specs)
    return Packets(np.concatenate(fr), np.concatenate(ln).astype(np.uint32), np.array(sid, np.uint32),
                   np.full(n, IFINDEX, np.uint32), np.array(lid, np.uint16), np.array(tci, np.uint8), np.array(fh, np.uint32))


def short(ev):
    """A decoded record in the KAT file's notation."""
    if ev["type"] == MON.NOTIFY_DBG_MSG:
        return [ev["name"], ev["arg1"], ev["arg2"], ev["arg3"]]
    if ev["type"] == MON.NOTIFY_DBG_CAPTURE:
        return [ev["name"], ev["arg1"]]
    if ev["type"] == MON.NOTIFY_TRACE:
        return [ev["name"], ev["reason"]]
    return ["DROP", ev["reason"]]


def run_anchored(sc, batches, nows, what=""):
    """The model over the batches, anchored: its verdicts and final CT maps must equal the C
    oracle's on the same input.  Returns (model, records per batch, notification lists per batch)."""
    model, ref = M.DbgModel(sc), OracleDP(sc)
    recs, evs = [], []
    for pk, now in zip(batches, nows):
        out, ev = model.batch(pk, ref.parse(pk), now)
        want = ref.ingress(pk, now)
        for f in ("action", "reason", "ct_ret", "flags", "proxy_port"):
            assert np.array_equal(out[f], want[f]), (what, f, out[f], want[f])
        recs.append(want)
        evs.append(ev)
    for name, m in model.ct.items():
        assert m.dump() == ref.dump(name), (what, name)
    return model, recs, evs


def test_kats_cover_the_cases():
    names = [c["name"] for c in kats()]
    assert len(names) == len(set(names)) >= 16 and all(c.get("ref") for c in kats())


def test_model_reproduces_every_kat():
    for c in kats():
        sc = scenario(ct=c.get("ct"), prefill=c.get("prefill", ()), px_max=c.get("px_max", 4096))
        # one call per packet: a sequence is two calls on the same maps
        batches = [packets([p]) for p in c["packets"]]
        _, recs, evs = run_anchored(sc, batches, [NOW] * len(batches), c["name"])
        got = [[short(e) for e in ev[0]] for ev in evs]
        assert got == c["expect"], (c["name"], got)
        for ev in evs:
            assert all(e["source"] == 100 for e in ev[0])          # EVENT_SOURCE = LXC_ID


def test_program_without_the_flag_sends_no_debug_record():
    sc = scenario(debug=())
    _, _, evs = run_anchored(sc, [packets(kats()[0]["packets"])], [NOW])
    assert [short(e) for e in evs[0][0]] == [["TRACE_TO_LXC", 0]]


def _slot(b):
    return b + bytes(MON.EVENT_RECORD - len(b))


def test_monitor_decodes_the_four_record_types():
    drop = _slot(struct.pack("<BBHIIIIIII", 1, 133, 100, 0xdead, 74, 74, 1000, 300, 100, 11) + bytes(range(74)))
    d = MON.decode(drop)
    assert (d["type"], d["reason"], d["source"], d["hash"], d["len_orig"], d["len_cap"], d["src_label"], d["dst_label"],
            d["dst_id"], d["ifindex"]) == (1, 133, 100, 0xdead, 74, 74, 1000, 300, 100, 11)
    assert d["data"] == bytes(range(74))
    trace = _slot(struct.pack("<BBHIIIIIHBBI", 4, 1, 100, 7, 200, 128, 300, 0, 0, 2, 0, 3) + bytes([9] * 128))
    d = MON.decode(trace)
    assert (d["name"], d["len_orig"], d["len_cap"], d["src_label"], d["dst_id"], d["reason"], d["ifindex"]) == \
        ("TRACE_TO_PROXY", 200, 128, 300, 0, 2, 3) and d["data"] == bytes([9] * 128)
    msg = _slot(struct.pack("<BBHIIII", 2, 8, 100, 5, 5300, 7, 0))
    d = MON.decode(msg)
    assert (d["name"], d["source"], d["hash"], d["arg1"], d["arg2"], d["arg3"]) == ("DBG_CT_MATCH", 100, 5, 5300, 7, 0)
    cap = _slot(struct.pack("<BBHIIIII", 3, 9, 100, 5, 60, 60, 39226, 0) + bytes([7] * 60))
    d = MON.decode(cap)
    assert (d["name"], d["len_orig"], d["len_cap"], d["arg1"], d["arg2"]) == ("DBG_CAPTURE_PROXY_POST", 60, 60, 39226, 0)
    assert d["data"] == bytes([7] * 60)                            # the capture starts at offset 24 (DebugCaptureLen)
    assert [x["type"] for x in MON.decode_ring(np.frombuffer(drop + trace + msg + cap, np.uint8), 3)] == [1, 4, 2]
    # the subtype numbers of bpf/lib/dbg.h that handle_policy uses
    idx = MON.DBG_NAMES.index
    assert (idx("DBG_GENERIC"), idx("DBG_POLICY_DENIED"), idx("DBG_CT_MATCH"), idx("DBG_CT_VERDICT"), idx("DBG_TO_HOST"),
            idx("DBG_REV_PROXY_UPDATE"), idx("DBG_L4_POLICY"), idx("DBG_CT_LOOKUP4_1"), idx("DBG_CT_CREATED4"),
            idx("DBG_CT_LOOKUP6_1"), idx("DBG_CT_CREATED6"), idx("DBG_SKIP_PROXY"), idx("DBG_L4_CREATE")) == \
        (1, 5, 8, 15, 19, 40, 41, 44, 46, 47, 49, 50, 51)
    assert MON.DBG_CAPTURE_NAMES.index("DBG_CAPTURE_PROXY_POST") == 9
