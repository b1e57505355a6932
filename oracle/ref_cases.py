"""The scenarios run through the executed reference programs — TEST INFRASTRUCTURE ONLY.

Shared by the recipe (oracle/refdiff.build), the fixture generator
(tests/golden/make_ref_golden.py) and the tests: a case name gives the same Scenario and
the same `now` per batch everywhere.  Inputs are regenerated from here, never stored.
"""
import numpy as np

from cilium_amd import synth
from cilium_amd.synth import (MapSpec, Packets, HASH, TCP, UDP, ICMP, ICMPV6, F_SYN, F_ACK, F_FIN, F_RST,
                              LXC_PRODUCTION, LB_L3, LB_L4, LB_REDIRECT, ip4)

PROGRAMS = ("lxc", "lb")
FUZZ = dict(n_ep=4, n_packets=2000, n_batches=2)
CASES = ("fuzz1", "fuzz2", "hand")
LXC_TRACE_NOTIFY = 64


def _node(sc):
    """cilium_proxy4/6 and the node_config.h values of the proxy redirect: the reference
    always has them, so every case does."""
    sc.add_map(MapSpec("cilium_proxy4", HASH, 10, 16, 524288, 0))
    sc.add_map(MapSpec("cilium_proxy6", HASH, 22, 28, 524288, 0))
    sc.node = {"proxy4": "cilium_proxy4", "proxy6": "cilium_proxy6", "ipv4_gateway": 0xfffff50a,
               "host_ip6": bytes([0xbe, 0xef, 0, 0, 0, 0, 0, 0, 0, 0, 0xa, 0, 0x2, 0xf, 0xff, 0xff]),
               "host_mac": bytes([0xce, 0x72, 0xa7, 0x03, 0x88, 0x56]),
               "node_mac": bytes([0xde, 0xad, 0xbe, 0xef, 0xc0, 0xde])}


def _checksums(sc, seed):
    """Random IPv4 header and L4 checksum fields (every tenth UDP / TCP one 0), so that the
    incremental checksum updates are compared on non-trivial words."""
    rng = np.random.default_rng(seed ^ 0xC5C5)
    for pk in sc.batches:
        f, m = pk.frames, pk.n
        v4 = (f[:, 12] == 0x08) & (f[:, 13] == 0x00)
        f[v4, 24:26] = rng.integers(0, 256, (int(v4.sum()), 2))
        l4 = 14 + (f[:, 14] & 0xf).astype(np.int64) * 4
        pr = f[:, 23]
        off = np.where(pr == 6, l4 + 16, np.where(pr == 17, l4 + 6, -1))
        ck = rng.integers(0, 65536, m)
        ck[rng.random(m) < 0.1] = 0
        ok = v4 & (off >= 0) & (off + 1 < f.shape[1])
        rows = np.nonzero(ok)[0]
        f[rows, off[ok]] = (ck[ok] >> 8).astype(np.uint8)
        f[rows, off[ok] + 1] = (ck[ok] & 0xff).astype(np.uint8)


def params(name):
    if name.startswith("fuzz"):
        return dict(FUZZ, kind="fuzz", seed=int(name[4:]))
    return dict(kind="hand")


def scenario(name):
    if name.startswith("fuzz"):
        seed = int(name[4:])
        sc = synth.fuzz(seed=seed, **FUZZ)
        _node(sc)
        _checksums(sc, seed)
        sc.name = "ref_" + name
        return sc
    if name == "hand":
        return hand()
    raise KeyError(name)


def nows(sc):
    """`now` advances per batch, as in the parity tests."""
    return [sc.now + i for i in range(len(sc.batches))]


# ------------------------------------------------------------------ the hand-built case
def hand():
    """At most 200 packets that force what a uniform fuzz reaches rarely; see the list in
    tests/test_ref_diff.py.  Two endpoints (2000: production flags + trace notifications and an
    L4 proxy list; 2001: production), one batch per `now` step.  sc.meta["expect"][batch] lists per
    packet what the reference is expected to do, worked out from its text: (action, drop reason,
    ct_ret or None where no trace notification shows it, what the packet is there for);
    sc.meta["boundary"] the CT entries probed at their lifetime boundary."""
    sc = synth.Scenario("ref_hand", now=5000)
    _node(sc)
    ep4 = np.array([ip4("10.1.0.1"), ip4("10.1.0.2")], np.uint32)
    ep6 = np.zeros((2, 16), np.uint8)
    ep6[:, 0:2] = (0xf0, 0x0d)
    ep6[0, 15], ep6[1, 15] = 1, 2
    rem = np.array([ip4("100.64.1.10"), ip4("100.64.1.11"), ip4("100.64.9.9"), ip4("100.64.1.12")], np.uint32)
    rem6 = np.zeros((2, 16), np.uint8)
    rem6[:, 0:4] = (0x20, 0x01, 0x0d, 0xb8)
    rem6[0, 15], rem6[1, 15] = 0x10, 0x11
    vip4 = np.array([ip4("10.96.0.1"), ip4("10.96.0.2"), ip4("10.96.0.3")], np.uint32)
    vip6 = np.zeros((1, 16), np.uint8)
    vip6[0, 0], vip6[0, 15] = 0xfd, 0x01
    # services: one backend; three backends (not a power of two); an IPv6 one with a rev-NAT index
    K, V = [], []
    for vip, port, backs, rn in ((vip4[0], 80, [(ep4[0], 8080)], 1), (vip4[1], 53, [(ep4[0], 53), (ep4[1], 5353), (ep4[1], 53)], 2),
                                 (vip4[2], 443, [(ep4[1], 443)] * 3, 3)):
        K.append(synth.lb4_keys([vip], [port], [0])); V.append(synth.lb4_vals([0], [0], [len(backs)], [0]))
        for s, (t, p) in enumerate(backs, 1):
            K.append(synth.lb4_keys([vip], [port], [s])); V.append(synth.lb4_vals([t], [p], [0], [rn]))
    sc.add_map(MapSpec("lb4_svc", HASH, 8, 12, 65536, 0, np.concatenate(K), np.concatenate(V)))
    K = [synth.lb6_keys(vip6, [80], [0]), synth.lb6_keys(vip6, [80], [1])]
    V = [synth.lb6_vals(np.zeros((1, 16), np.uint8), [0], [1], [0]), synth.lb6_vals(ep6[0:1], [8080], [0], [2])]
    sc.add_map(MapSpec("lb6_svc", HASH, 20, 24, 65536, 0, np.concatenate(K), np.concatenate(V)))
    sc.lb = {"lb4": "lb4_svc", "lb6": "lb6_svc", "flags": LB_L3 | LB_L4 | LB_REDIRECT, "redirect_ifindex": 1}
    rk, rv = synth.revnat4_entries([1, 2, 3], vip4, [80, 53, 443])
    sc.add_map(MapSpec("revnat4", HASH, 2, 6, 65536, 0, rk, rv))
    rk, rv = synth.revnat6_entries([2], vip6, [80])
    sc.add_map(MapSpec("revnat6", HASH, 2, 18, 65536, 0, rk, rv))
    # CT entries as the from-container program leaves them for a connection E:sport -> rem:80, which is
    # what a reply finds on ingress: key (daddr E, saddr rem, dport 80, sport, TCP, TUPLE_F_OUT)
    now = sc.now
    E = ep4[0]
    ek = synth.ct4_keys([E] * 4, [rem[0], rem[0], rem[3], rem[3]], synth.raw16([80] * 4),
                        synth.raw16([40000, 40002, 40001, 40003]), [TCP] * 4, [0] * 4)
    ev = synth.ct_vals(4, [now + 100, now + 100, now + 1, now + 1], 16, 0, 300, tx=(3, 300))
    ev[0, 38:40] = synth.le_bytes(synth.raw16([1]), "<u2")            # rev-NAT index 1: the reply is rewritten
    ev[1, 36:38] = 0                                                   # only the SYN seen so far
    rk = synth.ct4_keys([E], [rem[0]], [0], [0], [ICMP], [2])          # its related-ICMP entry (TUPLE_F_RELATED)
    sc.add_map(MapSpec("ct4", synth.LRU_HASH, 14, 48, 4096, 0, np.concatenate([ek, rk]),
                       np.concatenate([ev, synth.ct_vals(1, now + 100, 16)])))
    sc.add_map(MapSpec("ct6", synth.LRU_HASH, 40, 48, 4096, 0))
    sc.meta["boundary"] = [(bytes(ek[2]), 1), (bytes(ek[3]), 2)]       # (key, the batch that probes it)
    for e in range(2):
        kk = np.concatenate([synth.policy_keys([300, 300, 300], [80, 8081, 53], [TCP, TCP, UDP]),
                             synth.policy_keys([301], [0], [0]), synth.policy_keys([0], [9000], [TCP])])
        vv = np.concatenate([synth.policy_vals([0, 7777, 0]), synth.policy_vals([0]), synth.policy_vals([0])])
        sc.add_map(MapSpec("pol%d" % e, HASH, 8, 24, 16384, 0, kk, vv))
        ck, cv = synth.lpm_dedup(synth.lpm4_keys([24], [ip4("100.64.9.0")]), np.ones((1, 1), np.uint8), 32)
        sc.add_map(MapSpec("cidr4_%d" % e, synth.LPM, 8, 1, 1024, synth.NO_PREALLOC, ck, cv))
        # ipv6_policy hands policy_can_access_ingress &tuple.saddr after ct_lookup6 reversed the tuple of
        # a new flow: the CIDR6 lookup sees the endpoint's own address.  Endpoint 0's map holds that
        # address (the allow), endpoint 1's the remote prefix (which therefore does not allow).
        if e == 0:
            ck, cv = synth.lpm_dedup(synth.lpm6_keys([128], ep6[0:1]), np.ones((1, 1), np.uint8), 128)
        else:
            ck, cv = synth.lpm_dedup(synth.lpm6_keys([64], rem6[1:2].copy()), np.ones((1, 1), np.uint8), 128)
        sc.add_map(MapSpec("cidr6_%d" % e, synth.LPM, 20, 1, 1024, synth.NO_PREALLOC, ck, cv))
        sc.lxc.append({"lxc_id": 2000 + e, "seclabel": 256 + e, "policy": "pol%d" % e, "ct4": "ct4", "ct6": "ct6",
                       "cidr4": "cidr4_%d" % e, "cidr6": "cidr6_%d" % e, "revnat4": "revnat4", "revnat6": "revnat6",
                       "flags": LXC_PRODUCTION | (LXC_TRACE_NOTIFY if e == 0 else 0),
                       "l4": [(80, 15000, TCP), (53, 0, UDP)] if e == 0 else []})
    sc.host_ifindex = 3
    sc.meta["expect"] = []
    stride = 128
    F, L, SID, LID, W = [], [], [], [], []
    NEW, EST, REPLY, RELATED = 0, 1, 2, 3
    FWD, SHOT = 7, 2                    # delivered: redirect() to the entry ifindex (10) or, proxied, to HOST_IFINDEX

    def v4(want, s, d, pr, sp=0, dp=0, tf=0, it=0, sid=300, lid=2000, ck=None, **kw):
        f, ln = synth.frames_v4(1, stride, [s], [d], [pr], [sp], [dp], [tf], [it], **kw)
        if ck is not None:
            l4 = 14 + (int(f[0, 14]) & 0xf) * 4
            o = l4 + (16 if pr == TCP else 6)
            f[0, o], f[0, o + 1] = ck >> 8, ck & 0xff
        f[0, 24:26] = (0x12, 0x34)
        F.append(f[0]); L.append(int(ln[0])); SID.append(sid); LID.append(lid); W.append(want)

    def v6(want, s, d, nh, sp=0, dp=0, tf=0, it=0, sid=300, lid=2000, ext=None, **kw):
        f, ln = synth.frames_v6(1, stride, s[None, :], d[None, :], [nh], [sp], [dp], [tf], [it], ext=ext, **kw)
        F.append(f[0]); L.append(int(ln[0])); SID.append(sid); LID.append(lid); W.append(want)

    def batch():
        n = len(F)
        pk = Packets(np.array(F, np.uint8), np.array(L, np.uint32), np.array(SID, np.uint32),
                     np.full(n, 10, np.uint32), np.array(LID, np.uint16), np.zeros(n, np.uint8),
                     (np.arange(n, dtype=np.uint32) * 2654435761 & 0xffffffff).astype(np.uint32))
        sc.batches.append(pk)
        sc.meta["expect"].append(list(W))
        F.clear(); L.clear(); SID.clear(); LID.clear(); W.clear()

    E2 = ep4[1]
    # ---- batch 0 (now): a TCP life and the tuple reused, an RST, related ICMP, rev-NAT, CIDR, proxy ports
    v4((FWD, 0, NEW, "SYN: new, the L4 list's proxy port 15000"), rem[1], E, TCP, 41000, 80, F_SYN, ck=0xbeef)
    v4((FWD, 0, REPLY, "SYN-ACK answering the endpoint's own SYN"), rem[0], E, TCP, 80, 40002, F_SYN | F_ACK)
    v4((FWD, 0, EST, "ACK: established"), rem[1], E, TCP, 41000, 80, F_ACK, ck=0x0001)
    v4((FWD, 0, EST, "FIN: closing"), rem[1], E, TCP, 41000, 80, F_FIN | F_ACK)
    v4((FWD, 0, EST, "SYN on the closing tuple: reopened"), rem[1], E, TCP, 41000, 80, F_SYN)
    v4((FWD, 0, NEW, "the policy entry's own proxy port 7777"), rem[1], E, TCP, 41001, 8081, F_SYN)
    v4((FWD, 0, EST, "RST"), rem[1], E, TCP, 41001, 8081, F_RST)
    v4((FWD, 0, RELATED, "ICMP error related to the endpoint's live connection"), rem[0], E, ICMP, it=3)
    v4((SHOT, 133, None, "ICMP error towards an ingress-created flow: found by the reversed tuple, so "
        "ESTABLISHED, and policy denies it (the related entry is deleted)"), rem[1], E, ICMP, it=3)
    v4((FWD, 0, REPLY, "reply with a rev-NAT index: source rewritten to the VIP"), rem[0], E, TCP, 80, 40000, F_ACK,
       ck=0x1234)
    v4((FWD, 0, NEW, "CIDR-only allow (reserved identity, 100.64.9.0/24)"), rem[2], E, TCP, 1, 2, F_SYN, sid=2)
    v4((SHOT, 133, None, "the same from outside the CIDR"), rem[1], E, TCP, 1, 2, F_SYN, sid=2)
    v4((FWD, 0, NEW, "UDP checksum 0, allowed, L4 list entry without a proxy"), rem[1], E, UDP, 5000, 53, ck=0)
    v4((FWD, 0, NEW, "wildcard-identity L4 entry"), rem[1], E, TCP, 41002, 9000, F_SYN, sid=999)
    v4((FWD, 0, None, "L3-only allow on the second endpoint"), rem[1], E2, TCP, 41003, 80, F_SYN, sid=301, lid=2001)
    v4((SHOT, 133, None, "denied"), rem[1], E2, TCP, 41004, 80, F_SYN, sid=555, lid=2001)
    # IPv6: fragment header, nexthdr 59, extension chains, AUTH, a rev-NAT index in the destination
    e6, r6 = ep6[0], rem6[0]
    v6((FWD, 0, NEW, "IPv6 SYN: proxy port 15000"), r6, e6, TCP, 42000, 80, F_SYN)
    v6((SHOT, 137, None, "fragment header: ipv6_hdrlen's error is not tested, nexthdr stays 44"), r6, e6, TCP, 42000, 80,
       F_SYN, ext=[([44], [0])])
    v6((SHOT, 137, None, "nexthdr 59: likewise"), r6, e6, TCP, 42000, 80, F_SYN, ext=[([59], [0])])
    v6((FWD, 0, NEW, "three extension headers: the deepest chain that is walked"), r6, e6, TCP, 42001, 80, F_SYN,
       ext=[([0], [0]), ([60], [0]), ([43], [0])])
    v6((SHOT, 137, None, "four-deep chain: the walk gives up, nexthdr stays HOP"), r6, e6, TCP, 42002, 80, F_SYN,
       ext=[([0], [0]), ([60], [0]), ([43], [0]), ([60], [0])])
    v6((SHOT, 137, None, "five-deep chain: the same"), r6, e6, TCP, 42003, 80, F_SYN,
       ext=[([0], [0]), ([60], [0]), ([43], [0]), ([60], [0]), ([0], [0])])
    v6((FWD, 0, NEW, "AUTH header of 8 bytes: both length formulas agree"), r6, e6, UDP, 42004, 53, ext=[([51], [0])],
       payload=24)
    v6((SHOT, 133, None, "AUTH header of 12 bytes: its length is taken by the next header's formula (16), the "
        "ports are read 4 bytes late"), r6, e6, UDP, 42004, 53, ext=[([51], [1])], payload=24)
    d6 = e6.copy(); d6[12:14] = (0x02, 0x00)                         # s6_addr32[3] & 0xFFFF = rev-NAT index 2
    v6((FWD, 0, NEW, "rev-NAT index in the destination: zeroed, kept in the CT entry"), r6, d6, TCP, 42005, 80, F_SYN)
    v6((FWD, 0, NEW, "CIDR6 allow as written: the lookup sees the endpoint's own address"), rem6[1], e6, TCP, 1, 2,
       F_SYN, sid=2)
    v6((SHOT, 133, None, "a source inside the endpoint's CIDR6 prefix is not what the lookup sees"), rem6[1], ep6[1],
       TCP, 1, 2, F_SYN, sid=2, lid=2001)
    v6((SHOT, 133, None, "ICMPv6 echo request without a policy entry"), r6, e6, ICMPV6, it=128)
    # LB traffic (what handle_policy of endpoint 2000 makes of it is listed too): one backend; three
    # backends over several hashes; UDP checksum 0; the IPv6 service
    for k in range(6):
        v4((FWD, 0, NEW, "to the three-backend UDP service"), rem[1], vip4[1], UDP, 6000 + k, 53,
           ck=0 if k % 2 else 0x4321)
        v4((SHOT, 133, None, "to the three-backend TCP service"), rem[1], vip4[2], TCP, 6100 + k, 443, F_SYN, ck=0xffff)
    v4((FWD, 0, NEW, "to the one-backend service"), rem[1], vip4[0], TCP, 6200, 80, F_SYN, ck=0x8001)
    v6((FWD, 0, NEW, "to the IPv6 service"), r6, vip6[0], TCP, 6300, 80, F_SYN)
    batch()
    # ---- batch 1: now == lifetime of the first boundary entry; batch 2: now == lifetime + 1 of the second
    for sport in (40001, 40003):
        v4((FWD, 0, REPLY, "reply on the CT entry at its lifetime boundary"), rem[3], E, TCP, 80, sport, F_ACK)
        v4((FWD, 0, EST, "the reopened connection"), rem[1], E, TCP, 41000, 80, F_ACK)
        v4((FWD, 0, RELATED, "ICMP time exceeded related to the endpoint's connection"), rem[0], E, ICMP, it=11)
        batch()
    return sc
