"""The DebugLB endpoint option (LB_DEBUG, GF_LXC_F_LB_DEBUG): the reverse-NAT messages
handle_policy sends with DEBUG and LB_DEBUG.  The hand-derived known answers of
tests/golden/lbdbg_kats.json against the Python restatement (tests/lbdbg_model.py), the
model anchored on the C oracle (verdicts and final CT contents; the oracle runs the
reverse NAT), cilium_amd.monitor on hand-built records of the four subtypes, and the load
rules.  CPU only; the GPU side is tests/test_gpu_lb_debug.py."""
import ctypes as C
import ipaddress
import json
import os
import struct

import numpy as np

from cilium_amd import monitor as MON
from cilium_amd import synth
from cilium_amd.synth import Packets
from oracle.scenario import OracleDP
from tests import dbg_model as DM
from tests import lbdbg_model as M
from tests.test_debug_notify import (BASE_FLAGS, HOST_IFINDEX, IFINDEX, LXC_DEBUG, NOW, PROTO, SRC4, SRC6, ep_addr,
                                     short)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LXC_LB_DEBUG = synth.LXC_LB_DEBUG
BOTH = LXC_DEBUG | LXC_LB_DEBUG
VIP6 = ipaddress.IPv6Address("fd00::60:a").packed


def kats():
    with open(os.path.join(GOLDEN, "lbdbg_kats.json")) as f:
        return json.load(f)["cases"]


def src_addr(k):
    """Source k of a test (0: the KAT source) as (IPv4 host-order int, IPv6 bytes)."""
    s6 = bytearray(SRC6)
    s6[8] = k
    return SRC4 + (k << 8), bytes(s6)


def scenario(flags=(BOTH,), prefill=(), local=False):
    """len(flags) endpoints as in tests.test_debug_notify.scenario (LXC_ID 100 + k, SECLABEL 300 + k,
    10.1.0.1 + k / f00d::k:0:1, the KAT policy), endpoint k with BASE_FLAGS | flags[k], all bound to the KAT
    reverse-NAT maps.  prefill: CT entries {ep, src, family, sport, dport (the ports of the frame that
    matches), proto, lifetime, revnat (host order), ct_flags, forward} in endpoint ep's map (the shared
    one unless `local`)."""
    n_ep = len(flags)
    sc = synth.Scenario("lbdbg", now=NOW, host_ifindex=HOST_IFINDEX)
    sc.add_map(synth.MapSpec("cilium_proxy4", synth.HASH, 10, 16, 4096, 0))
    sc.add_map(synth.MapSpec("cilium_proxy6", synth.HASH, 22, 28, 4096, 0))
    sc.node = {"proxy4": "cilium_proxy4", "proxy6": "cilium_proxy6", "ipv4_gateway": 0xfffff50a,
               "host_ip6": bytes([0xbe, 0xef] + [0] * 13 + [1]), "host_mac": bytes([0xce, 0x72, 0xa7, 0x03, 0x88, 0x56]),
               "node_mac": bytes([0xde, 0xad, 0xbe, 0xef, 0xc0, 0xde])}
    rk, rv = synth.revnat4_entries([7, 8], [synth.ip4("10.96.0.10"), synth.ip4("10.96.0.11")], [80, 0])
    sc.add_map(synth.MapSpec("revnat4", synth.HASH, 2, 6, 64, 0, rk, rv))
    rk, rv = synth.revnat6_entries([7], np.frombuffer(VIP6, np.uint8)[None], [80])
    sc.add_map(synth.MapSpec("revnat6", synth.HASH, 2, 18, 64, 0, rk, rv))
    names4 = [f"ct4_{k}" if local else "ct4" for k in range(n_ep)]
    names6 = [f"ct6_{k}" if local else "ct6" for k in range(n_ep)]
    kv = {n: ([], []) for n in names4 + names6}
    u8 = lambda b: np.frombuffer(b, np.uint8)[None]
    for p in prefill:
        k = p.get("ep", 0)
        e4, e6 = ep_addr(k)
        s4, s6 = src_addr(p.get("src", 0))
        nh = PROTO[p["proto"]]
        fs, fd = synth.raw16([p["sport"]]), synth.raw16([p["dport"]])      # the matching frame's ports
        val = synth.ct_vals(1, p["lifetime"], p.get("ct_flags", 16), synth.raw16([p.get("revnat", 0)]), 300)
        fwd = bool(p.get("forward"))
        if p.get("family") == 6:
            # reply direction: the tuple as built from the frame; forward: reversed, TUPLE_F_IN
            key = synth.pack_rows(u8(s6 if fwd else e6), u8(e6 if fwd else s6), synth.le_bytes(fd if fwd else fs, "<u2"),
                                  synth.le_bytes(fs if fwd else fd, "<u2"), np.full((1, 1), nh, np.uint8),
                                  np.full((1, 1), 1 if fwd else 0, np.uint8), np.zeros((1, 2), np.uint8))
            kv[names6[k]][0].append(key); kv[names6[k]][1].append(val)
        else:
            key = synth.ct4_keys([s4], [e4], fd, fs, [nh], [1]) if fwd else synth.ct4_keys([e4], [s4], fs, fd, [nh], [0])
            kv[names4[k]][0].append(key); kv[names4[k]][1].append(val)
    cat = lambda a: np.concatenate(a) if a else None
    for n in dict.fromkeys(names4):
        sc.add_map(synth.MapSpec(n, synth.LRU_HASH, 14, 48, 4096, 0, cat(kv[n][0]), cat(kv[n][1])))
    for n in dict.fromkeys(names6):
        sc.add_map(synth.MapSpec(n, synth.LRU_HASH, 40, 48, 4096, 0, cat(kv[n][0]), cat(kv[n][1])))
    for k in range(n_ep):
        pk_ = synth.policy_keys([1000, 1000, 1000, 2000], [80, 8080, 53, 0], [synth.TCP, synth.TCP, synth.UDP, 0])
        sc.add_map(synth.MapSpec(f"pol{k}", synth.HASH, 8, 24, 1024, 0, pk_, synth.policy_vals([0, 15001, 0, 0])))
        sc.lxc.append({"lxc_id": 100 + k, "seclabel": 300 + k, "policy": f"pol{k}", "ct4": names4[k], "ct6": names6[k],
                       "revnat4": "revnat4", "revnat6": "revnat6", "flags": BASE_FLAGS | flags[k], "l4": []})
    return sc


def packets(specs):
    """specs: dicts {ep, src, family, id, proto, sport, dport, tcp_flags, l4_keep, ext} (ext: IPv6
    extension headers [[type, hdrlen], ...]; l4_keep: the frame ends that many bytes into the L4 header)."""
    fr, ln, sid, lid, fh = [], [], [], [], []
    for j, p in enumerate(specs):
        k = p.get("ep", 0)
        e4, e6 = ep_addr(k)
        s4, s6 = src_addr(p.get("src", 0))
        nh = PROTO[p["proto"]]
        sport, dport = p.get("sport", 40000), p.get("dport", 0)
        if p.get("family") == 6:
            ext = [(t, h) for t, h in p.get("ext", [])]
            f, l_ = synth.frames_v6(1, 128, np.frombuffer(s6, np.uint8)[None], np.frombuffer(e6, np.uint8)[None], nh, sport,
                                    dport, p.get("tcp_flags", 0), 0, ext=ext or None)
            l4 = 54 + sum((h + 1) << 3 for _, h in ext)
        else:
            f, l_ = synth.frames_v4(1, 128, s4, e4, nh, sport, dport, p.get("tcp_flags", 0), 0)
            l4 = 34
        if "l4_keep" in p:
            l_ = np.array([l4 + p["l4_keep"]], np.uint32)
        fr.append(f); ln.append(l_); sid.append(p["id"]); lid.append(100 + k); fh.append(0xabc00000 + j)
    n = len(specs)
    return Packets(np.concatenate(fr), np.concatenate(ln).astype(np.uint32), np.array(sid, np.uint32),
                   np.full(n, IFINDEX, np.uint32), np.array(lid, np.uint16), np.zeros(n, np.uint8), np.array(fh, np.uint32))


def run_anchored(sc, batches, nows, what="", model_cls=M.LbDbgModel):
    """The model over the batches, anchored: its verdicts and final CT maps must equal the C
    oracle's on the same input.  Returns (model, records per batch, notification lists per batch)."""
    model, ref = model_cls(sc), OracleDP(sc)
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


def without_flag(sc):
    """The same scenario with LB_DEBUG cleared on every program: what dbg_model's asserts allow is
    unchanged, so the parent behaviour of a batch without reverse NAT comes from dbg_model itself."""
    for e in sc.lxc:
        e["flags"] &= ~LXC_LB_DEBUG
    return sc


# ------------------------------------------------------------------ scenarios shared with the GPU tests
def kat_batch():
    """The KAT traffic as one batch over four endpoints: DEBUG | LB_DEBUG, DEBUG only, LB_DEBUG only,
    neither.  Every case goes to every endpoint, from a source of its own per case."""
    specs, prefill = [], []
    for ci, c in enumerate(kats()):
        for ep in range(4):
            prefill += [dict(q, ep=ep, src=ci + 1) for q in c["prefill"]]
            specs += [dict(p, ep=ep, src=ci + 1) for p in c["packets"]]
    return [BOTH, LXC_DEBUG, LXC_LB_DEBUG, 0], specs, prefill


def all_replies(n):
    """n packets, each a reverse-NAT reply of a flow of its own (index 7, 8 or the missing 9 in turn)."""
    specs = [dict(id=2000, proto="tcp", sport=1024 + k, dport=50000, tcp_flags=16, src=k % 200) for k in range(n)]
    prefill = [dict(sport=1024 + k, dport=50000, proto="tcp", lifetime=9000, revnat=7 + k % 3, src=k % 200) for k in range(n)]
    return specs, prefill


def alternating_group():
    """Six packets of one connection's bucket, reply and forward direction in turn: the reply
    entry carries index 7, the forward one index 8 (reported by CT_MATCH, no LB message)."""
    rep = dict(id=2000, proto="tcp", sport=80, dport=40000, tcp_flags=16)
    fwd = dict(id=1000, proto="tcp", sport=80, dport=40000, tcp_flags=16)
    # the forward entry of a frame with ports (80, 40000) is the reverse of the reply entry for the same frame:
    # one frame cannot be both, so the two directions are two entries on swapped addresses — same flow group
    prefill = [dict(sport=80, dport=40000, proto="tcp", lifetime=9000, revnat=7)]
    return [dict(rep), dict(fwd, sport=40000, dport=80), dict(rep), dict(fwd, sport=40000, dport=80), dict(rep),
            dict(fwd, sport=40000, dport=80)], prefill + [dict(sport=40000, dport=80, proto="tcp", lifetime=9000, revnat=8,
                                                                forward=True)]


def v6_mix():
    """IPv6: reply hit, reply miss, an ESTABLISHED packet with an index, and an extension-header
    frame whose rewrite fails after the messages."""
    specs = [dict(family=6, id=2000, proto="tcp", sport=8090, dport=50000, tcp_flags=16),
             dict(family=6, id=2000, proto="tcp", sport=8091, dport=50000, tcp_flags=16),
             dict(family=6, id=1000, proto="tcp", dport=80, tcp_flags=16),
             dict(family=6, id=2000, proto="tcp", sport=8092, dport=50000, tcp_flags=16, ext=[[0, 0]], l4_keep=16),
             dict(family=6, id=2000, proto="udp", sport=8093, dport=50000)]
    prefill = [dict(family=6, sport=8090, dport=50000, proto="tcp", lifetime=9000, revnat=7),
               dict(family=6, sport=8091, dport=50000, proto="tcp", lifetime=9000, revnat=9),
               dict(family=6, sport=40000, dport=80, proto="tcp", lifetime=9000, revnat=7, forward=True),
               dict(family=6, sport=8092, dport=50000, proto="tcp", lifetime=9000, revnat=7),
               dict(family=6, sport=8093, dport=50000, proto="udp", lifetime=9000, revnat=7)]
    return specs, prefill


def local_three():
    """Three endpoints with maps of their own (ConntrackLocal): replies and forward packets, IPv4 and IPv6."""
    specs, prefill = [], []
    for k in range(18):
        ep, fam = k % 3, (4, 6)[(k // 3) % 2]
        if k % 2:
            specs.append(dict(ep=ep, family=fam, id=2000, proto="tcp", sport=3000 + k, dport=50000, tcp_flags=16))
            prefill.append(dict(ep=ep, family=fam, sport=3000 + k, dport=50000, proto="tcp", lifetime=9000, revnat=7 + k % 3))
        else:
            specs.append(dict(ep=ep, family=fam, id=1000, proto="tcp", sport=4000 + k, dport=80, tcp_flags=2))
    return [BOTH, BOTH, LXC_DEBUG], specs, prefill


def lb_names(evs):
    return [e["name"] for e in evs if e.get("name", "").startswith("DBG_LB")]


# ------------------------------------------------------------------ tests
def test_kats_cover_the_cases():
    names = [c["name"] for c in kats()]
    assert len(names) == len(set(names)) >= 8 and all(c.get("ref") for c in kats())
    for need in ("v4_reply_hit_with_port", "v4_reply_hit_without_port", "v4_reply_index_misses_the_map",
                 "v4_reply_loopback_entry", "v4_established_with_index", "v6_established_with_index",
                 "v4_reply_rewrite_fails_after_the_messages"):
        assert need in names


def test_model_reproduces_every_kat():
    for c in kats():
        sc = scenario(prefill=c["prefill"])
        batches = [packets([p]) for p in c["packets"]]
        _, recs, evs = run_anchored(sc, batches, [NOW] * len(batches), c["name"])
        got = [[short(e) for e in ev[0]] for ev in evs]
        assert got == c["expect"], (c["name"], got)
        for ev in evs:
            assert all(e["source"] == 100 for e in ev[0])          # EVENT_SOURCE = LXC_ID


def test_flag_needs_debug_and_debug_alone_is_the_parent():
    """LB_DEBUG without DEBUG sends nothing (dbg.h:134-233); DEBUG without LB_DEBUG sends the
    parent's records: the KAT lists with the DBG_LB* entries taken out."""
    for c in kats():
        batches = [packets([p]) for p in c["packets"]]
        _, _, evs = run_anchored(scenario(flags=(LXC_LB_DEBUG,), prefill=c["prefill"]), batches, [NOW] * len(batches))
        assert all(e["type"] in (MON.NOTIFY_TRACE, MON.NOTIFY_DROP) for ev in evs for e in ev[0]), c["name"]
        _, _, evs = run_anchored(scenario(flags=(LXC_DEBUG,), prefill=c["prefill"]), batches, [NOW] * len(batches))
        got = [[short(e) for e in ev[0]] for ev in evs]
        assert got == [[x for x in per if not x[0].startswith("DBG_LB")] for per in c["expect"]], c["name"]


def test_model_equals_the_oracle_on_the_gpu_scenarios():
    flags, specs, prefill = kat_batch()
    _, _, evs = run_anchored(scenario(flags, prefill), [packets(specs)], [NOW], "kats")
    per_ep = {ep: sum(len(lb_names(ev)) for ev, s in zip(evs[0], specs) if s["ep"] == ep) for ep in range(4)}
    assert per_ep[0] == sum(len([x for x in per if x[0].startswith("DBG_LB")]) for c in kats() for per in c["expect"])
    assert per_ep[1] == per_ep[2] == per_ep[3] == 0
    for n in (1, 65):
        specs, prefill = all_replies(n)
        _, _, evs = run_anchored(scenario(prefill=prefill), [packets(specs)], [NOW], f"n{n}")
        assert all(lb_names(ev)[:1] == ["DBG_LB4_REVERSE_NAT_LOOKUP"] for ev in evs[0])
    specs, prefill = alternating_group()
    _, _, evs = run_anchored(scenario(prefill=prefill), [packets(specs)], [NOW], "group")
    assert [len(lb_names(ev)) for ev in evs[0]] == [2, 0, 2, 0, 2, 0]
    specs, prefill = v6_mix()
    _, recs, evs = run_anchored(scenario(prefill=prefill), [packets(specs)], [NOW], "v6")
    assert [len(lb_names(ev)) for ev in evs[0]] == [2, 1, 2, 2, 2] and recs[0]["reason"][3] == 154
    flags, specs, prefill = local_three()
    run_anchored(scenario(flags, prefill, local=True), [packets(specs)], [NOW], "local")


def test_flag_cleared_is_dbg_model_on_traffic_without_reverse_nat():
    """On a batch without reverse NAT the two models agree record for record (lbdbg_model adds
    nothing else), and with reverse NAT the flag-cleared scenario gives the lists without DBG_LB*."""
    specs = [dict(id=1000, proto="tcp", dport=80, tcp_flags=2, src=k) for k in range(4)]
    sc = scenario(flags=(BOTH,))
    _, _, a = run_anchored(sc, [packets(specs)], [NOW])
    _, _, b = run_anchored(without_flag(scenario(flags=(BOTH,))), [packets(specs)], [NOW], model_cls=DM.DbgModel)
    assert a == b


def _slot(b):
    return b + bytes(MON.EVENT_RECORD - len(b))


def test_monitor_decodes_the_four_subtypes():
    idx = MON.DBG_NAMES.index
    assert (idx("DBG_LB6_REVERSE_NAT_LOOKUP"), idx("DBG_LB6_REVERSE_NAT"), idx("DBG_LB4_REVERSE_NAT_LOOKUP"),
            idx("DBG_LB4_REVERSE_NAT")) == (26, 27, 32, 33)        # positions in the enum of bpf/lib/dbg.h:22-110
    cases = [(32, 0x0700, 0, "DBG_LB4_REVERSE_NAT_LOOKUP", "Reverse NAT lookup, index=7"),
             (33, 0x0a00600a, 0x5000, "DBG_LB4_REVERSE_NAT", "Performing reverse NAT, address=10.96.0.10 port=80"),
             (26, 0x0900, 0, "DBG_LB6_REVERSE_NAT_LOOKUP", "Reverse NAT lookup, index=9"),
             (27, 0x0a006000, 0xbb01, "DBG_LB6_REVERSE_NAT", "Performing reverse NAT, address.p4=a006000 port=443")]
    for sub, a1, a2, name, text in cases:
        d = MON.decode(_slot(struct.pack("<BBHIIII", 2, sub, 100, 0xabc00001, a1, a2, 0)))
        assert (d["type"], d["name"], d["source"], d["hash"], d["arg1"], d["arg2"], d["arg3"]) == \
            (MON.NOTIFY_DBG_MSG, name, 100, 0xabc00001, a1, a2, 0)
        assert MON.dbg_text(d) == text
    other = MON.decode(_slot(struct.pack("<BBHIIII", 2, 8, 100, 5, 5300, 7, 0)))
    assert MON.dbg_text(other) == "DBG_CT_MATCH"


def test_synth_lb_debug_sets_the_flag_on_chosen_endpoints():
    sc = scenario(flags=(LXC_DEBUG, LXC_DEBUG, 0))
    assert synth.lb_debug(sc, [100, 102]) == [100, 102]
    assert [bool(e["flags"] & LXC_LB_DEBUG) for e in sc.lxc] == [True, False, True]
    assert [bool(e["flags"] & LXC_DEBUG) for e in sc.lxc] == [True, True, False]
    assert synth.lb_debug(sc) == [100, 101, 102] and all(e["flags"] & LXC_LB_DEBUG for e in sc.lxc)
    assert LXC_LB_DEBUG == 1 << 9


def test_prog_load_accepts_the_flag():
    """LB_DEBUG alone, with DEBUG, and with NO_CONNTRACK (inert without DEBUG: no rule of its own) all
    load; DEBUG | NO_CONNTRACK stays refused with the new bit next to it (the library loads without a
    device)."""
    import errno
    from cilium_amd._lib import lib, gf_lxc_cfg
    for extra in (LXC_LB_DEBUG, BOTH, LXC_LB_DEBUG | synth.LXC_NO_CONNTRACK):
        cfg = gf_lxc_cfg()
        cfg.lxc_id, cfg.seclabel = 7, 300
        cfg.flags = synth.LXC_POLICY_INGRESS | synth.LXC_LXC_IPV4 | extra
        assert lib.gf_lxc_prog_load(C.byref(cfg)) > 0, extra
    cfg = gf_lxc_cfg()
    cfg.flags = synth.LXC_POLICY_INGRESS | synth.LXC_LXC_IPV4 | BOTH | synth.LXC_NO_CONNTRACK
    assert lib.gf_lxc_prog_load(C.byref(cfg)) == -errno.EOPNOTSUPP
