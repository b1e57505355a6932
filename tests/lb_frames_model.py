"""bpf_lb's from-netdev over raw frames, restated per frame from the reference
(carlanton/cilium 1.0.0-rc9) — TEST INFRASTRUCTURE ONLY.

The CPU oracle runs bpf_lb only as a stage of its pipeline and only with what that needs: it
cannot show the program's frames without LB_REDIRECT (the pipeline goes on into bpf_netdev) and
has no LB_DSTMAC.  The tests own this model for those; tests/test_lb_frames.py anchors it on the
oracle wherever the oracle can speak.  It follows the reference line by line, not libgpuflow's
kernels:

  bpf/bpf_lb.c:169-212          from_netdev: the ethertype switch (:176-192), send_drop_notify_error
                                (:194-195), LB_REDIRECT / LB_DSTMAC (:197-209), TC_ACT_OK (:211)
  bpf/bpf_lb.c:115-166          handle_ipv4      :58-111  handle_ipv6 (new_dst.p4 |= rev_nat_index :103-104)
  bpf/lib/common.h:67-87        revalidate_data: ETH_HLEN + sizeof(iphdr / ipv6hdr) within the frame
  bpf/lib/ipv4.h:45-48          ipv4_hdrlen      bpf/lib/ipv6.h:61-98  ipv6_hdrlen (AUTH's length is
                                chosen by the NEXT header, as written; neither handler tests the
                                result, so a rejected chain leaves nexthdr = ip6->nexthdr and l4_off
                                = ETH_HLEN + a negative DROP_* code)
  bpf/lib/lb.h:191-220          extract_l4_port (l4_load_port = skb_load_bytes: -EFAULT past the frame)
  bpf/lib/lb.h:349-395, 397-423 lb6_lookup_service, lb6_lookup_slave; lb6_xlate
  bpf/lib/lb.h:565-613, 615-659 lb4_lookup_service, lb4_lookup_slave; lb4_xlate
  bpf/lib/lb.h:109-188          lb_enforce_rehash, lb*_select_slave: (hash % count) + 1, hash an input column
  bpf/lib/l4.h:50-60            l4_modify_port   bpf/lib/csum.h:45-79  csum_l4_offset_and_flags, csum_l4_replace
  bpf/lib/eth.h                 eth_store_daddr(skb, mac, 0): skb_store_bytes of 6 bytes at offset 0
  bpf/lib/drop.h:47-107         send_drop_notify_error -> struct drop_notify with source, labels,
                                dst_id and ifindex 0, then min(len, TRACE_PAYLOAD_LEN) frame bytes

Kernel helper rules (net/core/filter.c) as tests/overlay_model.py lists them.  A frame is a snap:
bytes past it are not held (reads give 0, writes are dropped).  One deviation of the library is
restated here instead of the reference, as DESIGN.md documents it for the pipeline's LB stage: a
frame that lb4_xlate / lb6_xlate drops midway (L4 checksum field outside the frame) keeps its
bytes, where the kernel's skb already had the new daddr.
"""
import struct

import numpy as np

from tests import ctoff_model as M
from tests.overlay_model import Snap, csum_replace2, skb_load_ok

LB_OUT = np.dtype([("action", "u1"), ("reason", "u1"), ("slave", "<u2"), ("new_dport", "<u2"),
                   ("rev_nat", "<u2"), ("new_daddr4", "<u4")])

TC_ACT_OK, TC_ACT_SHOT, TC_ACT_REDIRECT = 0, 2, 7
EFAULT = 14
DROP_INVALID, DROP_WRITE_ERROR, DROP_UNKNOWN_L4 = 134, 141, 142   # bpf/lib/common.h:224-256 (as -DROP_*)
DROP_CSUM_L3, DROP_CSUM_L4, DROP_NO_SERVICE = 153, 154, 158
DROP_INVALID_EXTHDR, DROP_FRAG_NOSUPPORT = 156, 157
LB_F_L3, LB_F_L4, LB_F_REDIRECT, LB_F_NO_IPV4, LB_F_NO_IPV6 = 1, 2, 4, 8, 16   # include/gpuflow.h
IPPROTO_ICMP, IPPROTO_TCP, IPPROTO_UDP, IPPROTO_ICMPV6 = 1, 6, 17, 58
ETH_HLEN = 14
TRACE_PAYLOAD_LEN = 128


def r32(s, off):
    return s.r16(off) | (s.r16(off + 2) << 16)


def w32(s, off, v):
    s.w16(off, v & 0xffff)
    s.w16(off + 2, v >> 16)


def ipv6_hdrlen(s, length, nexthdr):
    """ipv6.h:61-98.  Returns (len or -DROP_*, nexthdr as the caller's variable is left)."""
    hl, nh = 40, nexthdr
    for _ in range(4):                                  # IPV6_MAX_HEADERS
        if nh == 59:
            return -DROP_INVALID_EXTHDR, nexthdr
        if nh == 44:
            return -DROP_FRAG_NOSUPPORT, nexthdr
        if nh in (0, 43, 51, 60):
            if not skb_load_ok(ETH_HLEN + hl, 2, length):
                return -DROP_INVALID, nexthdr
            onh, ohl = s.r8(ETH_HLEN + hl), s.r8(ETH_HLEN + hl + 1)
            nh = onh
            hl += (ohl + 2) << 2 if nh == 51 else (ohl + 1) << 3
            continue
        return hl, nh
    return -DROP_INVALID_EXTHDR, nexthdr


def l4_csum_replace(s, length, off, frm, to, size, mangled_0):
    """bpf_l4_csum_replace (inet_proto_csum_replace_by_diff for size 0, _replace2 for size 2;
    BPF_F_MARK_MANGLED_0; BPF_F_PSEUDO_HDR only matters for CHECKSUM_COMPLETE / PARTIAL skbs)."""
    if not M.l4_csum_replace_ok(off, length):
        return -EFAULT
    old = s.r16(off)
    if mangled_0 and not old:
        return 0
    new = M.csum_fold(M.csum_add(to, 0xffffffff ^ old)) if size == 0 else csum_replace2(old, frm, to)
    if mangled_0 and not new:
        new = 0xffff                                    # CSUM_MANGLED_0
    s.w16(off, new)
    return 0


class LbFramesModel:
    """sc.lb = {lb4, lb6, flags, redirect_ifindex[, dstmac]} over sc.maps."""

    def __init__(self, sc, flags=None, dstmac="sc"):
        lb = sc.lb
        self.flags = lb["flags"] if flags is None else flags
        self.dstmac = lb.get("dstmac") if isinstance(dstmac, str) else dstmac
        assert self.dstmac is None or self.flags & LB_F_REDIRECT   # LB_DSTMAC sits inside #ifdef LB_REDIRECT
        tab = lambda name: {} if not name or sc.maps[name].keys is None else \
            {bytes(k): bytes(v) for k, v in zip(sc.maps[name].keys, sc.maps[name].vals)}
        self.lb4, self.lb6 = tab(lb.get("lb4")), tab(lb.get("lb6"))

    # ---- lb.h:565-598 / :349-380
    def lookup_service(self, tab, addr, dport, cnt_off):
        """Returns (master value or None, key->dport as the lookup leaves it)."""
        if self.flags & LB_F_L4 and dport:
            v = tab.get(addr + struct.pack("<HH", dport, 0))
            if v is not None and struct.unpack_from("<H", v, cnt_off)[0]:
                return v, dport
            dport = 0                                   # key->dport = 0
        if self.flags & LB_F_L3:
            v = tab.get(addr + struct.pack("<HH", dport, 0))
            if v is not None and struct.unpack_from("<H", v, cnt_off)[0]:
                return v, dport
        return None, dport

    def extract_l4_port(self, s, length, nexthdr, l4_off):
        """lb.h:191-220.  Returns (ret, dport raw)."""
        if nexthdr in (IPPROTO_TCP, IPPROTO_UDP):
            if not skb_load_ok(l4_off + 2, 2, length):  # l4_load_port
                return -EFAULT, 0
            return 0, s.r16(l4_off + 2)
        if nexthdr in (IPPROTO_ICMP, IPPROTO_ICMPV6):
            return 0, 0
        return -DROP_UNKNOWN_L4, 0

    def xlate_ok(self, length, l4_off, nexthdr, key_dport, svc_port, v6):
        """What lb4_xlate / lb6_xlate would return, before any write (the kept deviation: see the
        module docstring).  lb4_xlate: lb.h:643-646, :648-657; lb6_xlate: :403-407, :409-420."""
        co = M.csum_offset(nexthdr)
        if (co or v6) and not M.l4_csum_replace_ok(l4_off + co, length):
            return -DROP_CSUM_L4
        if self.flags & LB_F_L4 and svc_port and key_dport != svc_port and nexthdr in (IPPROTO_TCP, IPPROTO_UDP):
            if not M.l4_csum_replace_ok(l4_off + co, length):       # l4.h:53-54
                return -DROP_CSUM_L4
            if not M.skb_store_ok(l4_off + 2, 2, length):           # l4.h:56-57
                return -DROP_WRITE_ERROR
        return 0

    def l4_rewrite(self, s, length, l4_off, nexthdr, diff, key_dport, svc_port, v6):
        co = M.csum_offset(nexthdr)
        udp = nexthdr == IPPROTO_UDP                    # csum.h:56-59 BPF_F_MARK_MANGLED_0
        if co or v6:                                    # lb6_xlate: `if (csum_off)`, a pointer: always
            l4_csum_replace(s, length, l4_off + co, 0, diff, 0, udp)
        new_dport = 0
        if self.flags & LB_F_L4 and svc_port and key_dport != svc_port and nexthdr in (IPPROTO_TCP, IPPROTO_UDP):
            l4_csum_replace(s, length, l4_off + co, key_dport, svc_port, 2, udp)   # l4_modify_port
            s.w16(l4_off + 2, svc_port)
            new_dport = svc_port
        return new_dport

    def handle_ipv4(self, s, length, h):
        """bpf_lb.c:115-166.  Returns (ret, record fields dict, nd6)."""
        if length < ETH_HLEN + 20:                      # revalidate_data
            return -DROP_INVALID, {}, None
        nexthdr = s.r8(23)
        addr = bytes(s.f[30:34])
        l4_off = ETH_HLEN + (s.r8(14) & 0xf) * 4        # ipv4_hdrlen
        dport = 0
        if self.flags & LB_F_L4:
            ret, dport = self.extract_l4_port(s, length, nexthdr, l4_off)
            if ret == -DROP_UNKNOWN_L4:
                return TC_ACT_OK, {}, None
            if ret < 0:
                return ret, {}, None
        svc, dport = self.lookup_service(self.lb4, addr, dport, 6)
        if svc is None:
            return TC_ACT_OK, {}, None
        count = struct.unpack_from("<H", svc, 6)[0]
        slave = (h % count + 1) & 0xffff                # lb4_select_slave
        be = self.lb4.get(addr + struct.pack("<HH", dport, slave))
        if be is None:
            return -DROP_NO_SERVICE, {}, None
        target, port, _cnt, rev_nat = struct.unpack_from("<IHHH", be, 0)
        ret = self.xlate_ok(length, l4_off, nexthdr, dport, port, False)
        if ret < 0:
            return ret, {}, None
        old = r32(s, 30)
        w32(s, 30, target)                              # skb_store_bytes(daddr) :626
        diff = M.csum_add(M.csum_add(0, 0xffffffff ^ old), target)   # csum_diff(&key->address, 4, new_daddr, 4, 0)
        ck = s.r16(24)
        s.w16(24, M.csum_fold(M.csum_add(diff, 0xffffffff ^ ck)))    # l3_csum_replace(check, 0, sum, 0) :640
        nd = self.l4_rewrite(s, length, l4_off, nexthdr, diff, dport, port, False)
        return TC_ACT_REDIRECT, dict(slave=slave, new_dport=nd, rev_nat=rev_nat, new_daddr4=target), None

    def handle_ipv6(self, s, length, h):
        """bpf_lb.c:58-111."""
        if length < ETH_HLEN + 40:
            return -DROP_INVALID, {}, None
        addr = bytes(s.f[38:54])
        hl, nexthdr = ipv6_hdrlen(s, length, s.r8(20))
        l4_off = ETH_HLEN + hl
        dport = 0
        if self.flags & LB_F_L4:
            ret, dport = self.extract_l4_port(s, length, nexthdr, l4_off)
            if ret == -DROP_UNKNOWN_L4:
                return TC_ACT_OK, {}, None
            if ret < 0:
                return ret, {}, None
        svc, dport = self.lookup_service(self.lb6, addr, dport, 18)
        if svc is None:
            return TC_ACT_OK, {}, None
        count = struct.unpack_from("<H", svc, 18)[0]
        slave = (h % count + 1) & 0xffff
        be = self.lb6.get(addr + struct.pack("<HH", dport, slave))
        if be is None:
            return -DROP_NO_SERVICE, {}, None
        t = list(struct.unpack_from("<4I", be, 0))
        port, _cnt, rev_nat = struct.unpack_from("<HHH", be, 16)
        if rev_nat:
            t[3] |= rev_nat                             # new_dst.p4 |= svc->rev_nat_index :103-104
        ret = self.xlate_ok(length, l4_off, nexthdr, dport, port, True)
        if ret < 0:
            return ret, {}, None
        diff = 0
        for k in range(4):                              # ipv6_store_daddr + csum_diff(key->address, 16, new_dst, 16, 0)
            old = r32(s, 38 + 4 * k)
            w32(s, 38 + 4 * k, t[k])
            diff = M.csum_add(M.csum_add(diff, 0xffffffff ^ old), t[k])
        nd = self.l4_rewrite(s, length, l4_off, nexthdr, diff, dport, port, True)
        return TC_ACT_REDIRECT, dict(slave=slave, new_dport=nd, rev_nat=rev_nat, new_daddr4=0), struct.pack("<4I", *t)

    def frame(self, row, length, h):
        """from_netdev (bpf_lb.c:169-212) on one frame; row (uint8 [stride]) is rewritten in place.
        Returns (record tuple in LB_OUT order, new_daddr6 bytes)."""
        s = Snap(row, length)
        et = (s.r8(12) << 8) | s.r8(13) if length >= ETH_HLEN else 0     # skb->protocol
        ret, fields, nd6 = TC_ACT_OK, {}, None
        if et == 0x86DD and not self.flags & LB_F_NO_IPV6:
            ret, fields, nd6 = self.handle_ipv6(s, length, h)
        elif et == 0x0800 and not self.flags & LB_F_NO_IPV4:
            ret, fields, nd6 = self.handle_ipv4(s, length, h)
        if ret < 0:                                     # send_drop_notify_error(skb, ret, TC_ACT_SHOT)
            return (TC_ACT_SHOT, -ret, 0, 0, 0, 0), bytes(16)
        action = TC_ACT_OK
        if self.flags & LB_F_REDIRECT and ret == TC_ACT_REDIRECT:
            if self.dstmac is not None:                 # eth_store_daddr(skb, mac.addr, 0): cannot fail here,
                s.wbytes(0, self.dstmac)                # and `ret` is not what the program returns
            action = TC_ACT_REDIRECT                    # return redirect(ifindex, 0)
        f = fields
        return (action, 0, f.get("slave", 0), f.get("new_dport", 0), f.get("rev_nat", 0), f.get("new_daddr4", 0)), \
            nd6 or bytes(16)

    def batch(self, pk):
        """Returns (records LB_OUT [n], new_daddr6 [n,16] u8, frames as the program left them)."""
        frames = np.array(pk.frames, np.uint8, copy=True)
        recs = np.zeros(pk.n, LB_OUT)
        nd6 = np.zeros((pk.n, 16), np.uint8)
        for i in range(pk.n):
            h = int(pk.flow_hash[i]) if pk.flow_hash is not None else 0
            rec, n6 = self.frame(frames[i], int(pk.lens[i]), h)
            recs[i] = rec
            nd6[i] = np.frombuffer(n6, np.uint8)
        return recs, nd6, frames


def drop_events(pk, recs, frames):
    """send_drop_notify_error's ring records of the batch's TC_ACT_SHOT frames, in batch order
    ([k, 160] u8): struct drop_notify {type CILIUM_NOTIFY_DROP = 1, subtype = reason, source 0,
    hash, len_orig, len_cap, src_label 0, dst_label 0, dst_id 0, ifindex 0} + the captured bytes."""
    ev = []
    for i in np.nonzero(recs["action"] == TC_ACT_SHOT)[0]:
        length = int(pk.lens[i])
        cap = min(length, TRACE_PAYLOAD_LEN)
        r = np.zeros(160, np.uint8)
        h = int(pk.flow_hash[i]) if pk.flow_hash is not None else 0
        r[:32] = np.frombuffer(struct.pack("<8I", 1 | (int(recs["reason"][i]) << 8), h, length, cap, 0, 0, 0, 0), np.uint8)
        k = min(cap, frames.shape[1])
        r[32:32 + k] = frames[i, :k]
        ev.append(r)
    return np.array(ev, np.uint8).reshape(-1, 160)


# ---- checksum verification (RFC 1071 / 1624), for the tests
def ones_sum(b):
    if len(b) & 1:
        b = b + b"\0"
    x = sum(struct.unpack(f">{len(b) // 2}H", b))
    while x >> 16:
        x = (x & 0xffff) + (x >> 16)
    return x


def ip4_header_ok(f):
    ihl = (f[14] & 0xf) * 4
    return ones_sum(bytes(f[14:14 + ihl])) == 0xffff


def l4_ok(f, length):
    """The TCP / UDP checksum of a whole (untruncated, in-snap) IPv4 or IPv6 frame verifies."""
    f = bytes(f[:length])
    if f[12:14] == b"\x08\x00":
        l4, proto = 14 + (f[14] & 0xf) * 4, f[23]
        pseudo = f[26:34] + struct.pack(">BBH", 0, proto, length - l4)
    else:
        l4, proto = 54, f[20]
        pseudo = f[22:54] + struct.pack(">IBBBB", length - l4, 0, 0, 0, proto)
    return ones_sum(pseudo + f[l4:]) == 0xffff


def set_checksums(f, length):
    """Fills in correct IPv4 header and TCP / UDP checksums (IPv6 without extension headers)."""
    v4 = bytes(f[12:14]) == b"\x08\x00"
    if v4:
        ihl = (f[14] & 0xf) * 4
        f[24:26] = 0
        f[24:26] = np.frombuffer(struct.pack(">H", 0xffff ^ ones_sum(bytes(f[14:14 + ihl]))), np.uint8)
        l4, proto = 14 + ihl, int(f[23])
    else:
        l4, proto = 54, int(f[20])
    co = {6: 16, 17: 6}.get(proto)
    if co is None:
        return
    f[l4 + co:l4 + co + 2] = 0
    b = bytes(f[:length])
    pseudo = (b[26:34] + struct.pack(">BBH", 0, proto, length - l4)) if v4 else \
        (b[22:54] + struct.pack(">IBBBB", length - l4, 0, 0, 0, proto))
    c = 0xffff ^ ones_sum(pseudo + b[l4:])
    if proto == 17 and c == 0:
        c = 0xffff
    f[l4 + co:l4 + co + 2] = np.frombuffer(struct.pack(">H", c), np.uint8)


# ---- tests/golden/lb_frames_kats.json
def load_kats():
    import json
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lb_frames_kats.json")) as f:
        return json.load(f)


def kat_scenario(doc, flags, dstmac):
    """The KAT file's two service maps under one program configuration."""
    from cilium_amd import synth
    sc = synth.Scenario("lb_frames_kats")
    rows = lambda ent, j: np.array([list(bytes.fromhex(e[j])) for e in ent], np.uint8)
    sc.add_map(synth.MapSpec("lb4_svc", synth.HASH, 8, 12, 1024, 0, rows(doc["lb4"], 0), rows(doc["lb4"], 1)))
    sc.add_map(synth.MapSpec("lb6_svc", synth.HASH, 20, 24, 1024, 0, rows(doc["lb6"], 0), rows(doc["lb6"], 1)))
    sc.lb = {"lb4": "lb4_svc", "lb6": "lb6_svc", "flags": flags, "redirect_ifindex": 5}
    if dstmac is not None:
        sc.lb["dstmac"] = bytes.fromhex(dstmac)
    return sc


def kat_packets(doc, kats):
    """(Packets of the KATs' frames, expected records, expected new_daddr6, expected frames)."""
    from cilium_amd.synth import Packets
    n, S = len(kats), doc["stride"]
    f, out = np.zeros((n, S), np.uint8), np.zeros((n, S), np.uint8)
    recs, nd6 = np.zeros(n, LB_OUT), np.zeros((n, 16), np.uint8)
    for i, k in enumerate(kats):
        b, o = bytes.fromhex(k["frame"]), bytes.fromhex(k["out"])
        f[i, :len(b)] = list(b)
        out[i, :len(o)] = list(o)
        r = k["record"]
        recs[i] = tuple(r[name] for name in LB_OUT.names)
        nd6[i] = list(bytes.fromhex(k["new_daddr6"]))
    pk = Packets(f, np.array([k["len"] for k in kats], np.uint32), flow_hash=np.array([k["hash"] for k in kats], np.uint32))
    return pk, recs, nd6, out


def kat_groups(doc):
    """The KATs grouped by program configuration: [((flags, dstmac), [kat, ...]), ...]."""
    g = {}
    for k in doc["kats"]:
        g.setdefault((k["flags"], k["dstmac"]), []).append(k)
    return sorted(g.items(), key=lambda kv: (kv[0][0], kv[0][1] or ""))
