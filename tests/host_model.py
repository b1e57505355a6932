"""from-host, bpf_netdev.c compiled with -DFROM_HOST (the program on cilium_host), restated
per packet from the reference (carlanton/cilium 1.0.0-rc9) — TEST INFRASTRUCTURE ONLY.

The CPU oracle cannot express FROM_HOST, so the tests own this model of the program's front
(everything before the cilium_policy tail call); handle_policy of the delivered packets is
the unchanged oracle's (OracleDP.ingress) or tests/ctoff_model.py.  It follows the reference
line by line, not libgpuflow's kernels:

  bpf/bpf_netdev.c:414-468      from_netdev (FROM_HOST, ENABLE_IPV4; HANDLE_NS undefined)
  bpf/bpf_netdev.c:128-145      handle_identity_from_proxy
  bpf/bpf_netdev.c:328-396      handle_ipv4        :163-246  handle_ipv6
  bpf/bpf_netdev.c:264-325      reverse_proxy      :67-124   reverse_proxy6
  bpf/bpf_netdev.c:148-160      rewrite_dmac_to_host
  bpf/bpf_netdev.c:50-64, 249-261   derive_sec_ctx, derive_ipv4_sec_ctx
  bpf/lib/common.h:267-281      MARK_MAGIC_PROXY_*, get_identity_via_proxy; :289 TC_INDEX_F_SKIP_PROXY
  bpf/lib/common.h:445-475      proxy{4,6}_tbl_key / _value
  bpf/lib/l4.h:50-60            l4_modify_port
  bpf/lib/csum.h:45-79          csum_l4_offset_and_flags, csum_l4_replace
  bpf/lib/encap.h:30-70         encap_and_redirect
  bpf/lib/l3.h:106-164          ipv{6,4}_local_delivery (tests/overlay_model.py's restatement)

ENCAP_IFINDEX is defined iff the scenario's node has a non-zero encap_ifindex.  The model
reads the proxy maps as they are handed to front(): the state at the start of the call (a
reverse lookup never sees what handle_policy of the same call inserts later; on a CPU the
program runs packet by packet, the library documents the batch order).  skb->mark's reset
to 0 (:143) has no output.  Kernel helper rules as tests/overlay_model.py lists them; a frame
is a snap: bytes past it are not held (reads give 0, writes are dropped).
"""
import struct

import numpy as np

from cilium_amd.synth import Packets
from tests import ctoff_model as M
from tests import overlay_model as OM
from tests.overlay_model import PIPE_OUT, Snap, TAILCALL, ICMP6_TE

TC_ACT_OK, TC_ACT_SHOT, TC_ACT_REDIRECT = 0, 2, 7
DROP_INVALID, DROP_CT_INVALID_HDR, DROP_WRITE_ERROR = 134, 135, 141    # common.h:224-256 (as -DROP_*)
STAGE_POLICY, STAGE_HOST = 4, 7                                         # include/gpuflow.h
F_REV_PROXY, F_ICMP6_TE, F_PORTMAP = 0x10, 0x20, 0x80
MARK_MAGIC_PROXY_MASK, MARK_MAGIC_PROXY_INGRESS, MARK_MAGIC_PROXY_EGRESS = 0xFFF, 0xFEA, 0xFEB   # common.h:267-269
TC_INDEX_F_SKIP_PROXY = 1                                               # common.h:289
HOST_ID, WORLD_ID = 1, 2                                                # node_config.h:34-35
NETDEV_F_FIXED_SECCTX = 1
ENCAP = "encap"
TRACE_FROM_PROXY, TRACE_FROM_HOST = 6, 7                                # lib/trace.h:43-44


def r32(s, off):
    return s.r16(off) | (s.r16(off + 2) << 16)


def w32(s, off, v):
    s.w16(off, v & 0xffff)
    s.w16(off + 2, v >> 16)


def csum_replace4(check, old, new):
    """csum_replace4 / inet_proto_csum_replace4 on a received frame (include/net/checksum.h,
    net/core/utils.c): csum_fold(csum_add(csum_sub(~csum_unfold(check), from), to))."""
    return OM.csum_replace2(check, old, new)


def l4_csum_replace(s, off, frm, to, size, mangled_0):
    """bpf_l4_csum_replace (net/core/filter.c) after its offset check: size 0 by diff, 2 / 4
    inet_proto_csum_replace{2,4}; BPF_F_MARK_MANGLED_0 leaves a zero checksum alone and turns
    a zero result into 0xffff.  A field outside the snap is not held."""
    if off + 2 > s.cap:
        return
    old = s.r16(off)
    if mangled_0 and not old:
        return
    if size == 0:
        new = M.csum_fold(M.csum_add(to, 0xffffffff ^ old))
    else:
        new = csum_replace4(old, frm, to)
    if mangled_0 and not new:
        new = 0xffff
    s.w16(off, new)


def identity_from_proxy(mark):
    """handle_identity_from_proxy (:128-145).  Returns (proxy_identity, tc_index bits)."""
    magic = mark & MARK_MAGIC_PROXY_MASK
    if magic == MARK_MAGIC_PROXY_INGRESS:               # :135-137
        return mark >> 16, TC_INDEX_F_SKIP_PROXY
    if magic == MARK_MAGIC_PROXY_EGRESS:                # :138-139
        return mark >> 16, 0
    return 0, 0


def trace_first(mark):
    """from_netdev's send_trace_notify (:423-433): (observation point, src_label)."""
    pid, _ = identity_from_proxy(mark)
    return (TRACE_FROM_PROXY, pid) if pid else (TRACE_FROM_HOST, HOST_ID)


class HostModel:
    def __init__(self, sc):
        self.sc = sc
        ho = sc.host
        self.eps = OM.endpoints(sc, ho["lxc_map"])
        self.flags = ho.get("flags", 0)
        self.fixed = ho.get("fixed_secctx", 0)          # FIXED_SRC_SECCTX
        self.router = bytes(ho.get("router_ip6", bytes(16)))   # ROUTER_IP (derive_sec_ctx)
        self.net_mac = bytes(ho.get("cilium_net_mac", bytes(6)))   # CILIUM_NET_MAC
        nd = sc.node or {}
        self.encap_ifindex = nd.get("encap_ifindex", 0)  # ENCAP_IFINDEX, 0 = undefined
        self.cluster_range, self.cluster_mask = nd.get("ipv4_cluster_range", 0), nd.get("ipv4_cluster_mask", 0)
        self.ipv4_mask = nd.get("ipv4_mask", 0)
        self.node_router = bytes(nd.get("router_ip6", bytes(16)))
        tm = sc.maps.get(nd.get("tunnel_map")) if nd.get("tunnel_map") else None
        self.tunnel = {}
        if tm is not None and tm.keys is not None:
            self.tunnel = {bytes(k): bytes(v) for k, v in zip(tm.keys, tm.vals)}

    # ---- reverse_proxy (:264-325) / reverse_proxy6 (:67-124)
    def reverse_proxy(self, s, length, v6, l4_off, nh, table):
        """Returns (ret, translated)."""
        if nh not in (M.IPPROTO_TCP, M.IPPROTO_UDP):    # :276-286 / :79-89
            return 0, False
        if not OM.skb_load_ok(l4_off, 4, length):       # :280-281 / :83-84
            return -DROP_CT_INVALID_HDR, False
        ports = bytes(s.r8(l4_off + k) for k in range(4))     # key.dport = sport, key.sport = dport
        daddr = bytes(s.r8((38 if v6 else 30) + k) for k in range(16 if v6 else 4))
        val = table.get(daddr + ports + bytes([nh, 0]))       # :293 / :95
        if val is None:
            return 0, False
        alen = 16 if v6 else 4
        old_saddr = r32(s, 26)                                # :272, read at entry (an IHL < 5 puts l4_off inside the header)
        new_sport, = struct.unpack_from("<H", val, alen)      # raw be16
        old_sport = s.r16(l4_off)
        co = M.csum_offset(nh)
        mangled_0 = nh == M.IPPROTO_UDP                       # csum.h:56-59
        # l4_modify_port (:304 / :103): csum_l4_replace, then the 2-byte store
        if not M.l4_csum_replace_ok(l4_off + co, length):
            return -DROP_WRITE_ERROR, False                   # :305 / :105
        l4_csum_replace(s, l4_off + co, old_sport, new_sport, 2, mangled_0)
        s.w16(l4_off, new_sport)
        if not v6:
            new_saddr, = struct.unpack_from("<I", val, 0)
            w32(s, 26, new_saddr)                             # :307
            s.w16(24, csum_replace4(s.r16(24), old_saddr, new_saddr))   # :310 l3_csum_replace(.., 4)
            l4_csum_replace(s, l4_off + co, old_saddr, new_saddr, 4, mangled_0)   # :313-314
        else:
            diff = 0
            for k in range(4):                                # :107 ipv6_store_saddr, :112 csum_diff
                old = r32(s, 22 + 4 * k)
                new, = struct.unpack_from("<I", val, 4 * k)
                w32(s, 22 + 4 * k, new)
                diff = M.csum_add(M.csum_add(diff, 0xffffffff ^ old), new)
            l4_csum_replace(s, l4_off + co, 0, diff, 0, mangled_0)      # :114
        return 0, True                                        # :320 / :121 (the caller sets SKIP_PROXY)

    def encap(self, key):
        """encap_and_redirect (encap.h:30-70): bpf_tunnel_key.remote_ipv4, or None
        (DROP_NO_TUNNEL_ENDPOINT, which the callers turn into TC_ACT_OK)."""
        v = self.tunnel.get(key)
        if v is None:
            return None
        return struct.unpack_from(">I", v, 0)[0]              # bpf_htonl(tunnel->ip4) (:42)

    def packet(self, s, length, ethertype, nexthdr, l4_off, mark, proxy4, proxy6):
        """from_netdev (:414-468) up to the tail call.  Returns a dict: ret (a TC_ACT_* /
        negative DROP_*, or TAILCALL / ICMP6_TE / ENCAP), ep, mapped, secctx, tc (tc_index
        bits set), rev, tunnel."""
        pid, tc = identity_from_proxy(mark)                   # :425
        o = dict(ret=TC_ACT_OK, ep=None, mapped=None, secctx=0, tc=tc, rev=False, tunnel=0)
        if ethertype == 0x86DD:                               # :440-448 handle_ipv6
            if length < 54:                                   # :174-175
                o["ret"] = -DROP_INVALID
                return o
            if self.flags & NETDEV_F_FIXED_SECCTX:            # :53-54
                sec = self.fixed
            elif bytes(s.f[22:30]) == self.router[:8]:        # :56-60
                sec = struct.unpack(">I", bytes(s.f[14:18]))[0] & 0x000FFFFF
            else:
                sec = WORLD_ID
            if pid:                                           # :195-196
                sec = pid
            r, rev = self.reverse_proxy(s, length, True, l4_off, s.r8(20), proxy6)    # :198 ip6->nexthdr
            if r < 0:
                o["ret"] = r
                return o
            s.wbytes(0, self.net_mac)                         # :205
            ep = self.eps.get(bytes(s.f[38:54]) + bytes([2, 0, 0, 0]))   # :216
            if ep is None:
                if self.encap_ifindex and bytes(s.f[38:50]) == self.node_router[:12]:   # :225-227
                    t = self.encap(bytes(s.f[38:50]) + bytes(4) + bytes([2, 0, 0, 0]))   # :228-239
                    if t is not None:
                        o.update(ret=ENCAP, tunnel=t)
            elif not ep["flags"] & OM.ENDPOINT_F_HOST:        # :219-222
                r = OM.ipv6_l3(s, ep["node_mac"], ep["mac"])
                o["ret"] = r if r != TC_ACT_OK else TAILCALL
        elif ethertype == 0x0800:                             # :451-453 -> handle_ipv4
            if length < 34:                                   # :337-338
                o["ret"] = -DROP_INVALID
                return o
            sec = self.fixed if self.flags & NETDEV_F_FIXED_SECCTX else WORLD_ID   # :251-259
            if pid:                                           # :348-349
                sec = pid
            r, rev = self.reverse_proxy(s, length, False, l4_off, s.r8(23), proxy4)   # :351
            if r < 0:
                o["ret"] = r
                return o
            s.wbytes(0, self.net_mac)                         # :358
            ep = self.eps.get(bytes(s.f[30:34]) + bytes(12) + bytes([1, 0, 0, 0]))   # :369
            if ep is None:
                da = r32(s, 30)
                if self.encap_ifindex and (da & self.cluster_mask) == self.cluster_range:   # :380
                    t = self.encap(struct.pack("<I", da & self.ipv4_mask) + bytes(12) + bytes([1, 0, 0, 0]))
                    if t is not None:                         # :389-391
                        o.update(ret=ENCAP, tunnel=t)
            elif not ep["flags"] & OM.ENDPOINT_F_HOST:        # :372-375
                r = OM.ipv4_l3(s, ep["node_mac"], ep["mac"])
                o["ret"] = r if r != TC_ACT_OK else TAILCALL
        else:
            return o                                          # :462-464
        o.update(secctx=sec, rev=rev)
        if rev:
            o["tc"] |= TC_INDEX_F_SKIP_PROXY
        if o["ret"] == TAILCALL:
            r, mapped = OM.map_lxc_in(s, length, l4_off, ep, nexthdr)   # l3.h:123, 153
            o["mapped"] = mapped
            if r < 0:
                o["ret"] = r
            else:
                o["ep"] = ep
        return o

    def front(self, pk, cols, proxy4, proxy6):
        """Returns (front records PIPE_OUT, rewritten frames, delivered indices, the delivered
        subset as Packets: src_identity = secctx, ifindex / lxc_id from the endpoint entry,
        tc_index with the program's SKIP_PROXY bit)."""
        n = pk.n
        rec = np.zeros(n, PIPE_OUT)
        frames = pk.frames.copy()
        sid, ifx, lid = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.uint16)
        tci = np.zeros(n, np.uint8) if pk.tc_index is None else pk.tc_index.astype(np.uint8).copy()
        dl = []
        self.secctx = np.zeros(n, np.uint32)             # every packet's secctx (the event checks' labels)
        for i in range(n):
            length = int(pk.lens[i])
            s = Snap(frames[i], length)
            mark = 0 if pk.mark is None else int(pk.mark[i])
            p = self.packet(s, length, int(cols["ethertype"][i]), int(cols["proto"][i]), int(cols["l4_off"][i]), mark,
                            proxy4, proxy6)
            r = p["ret"]
            self.secctx[i] = p["secctx"]
            o = rec[i]
            o["stage"] = STAGE_HOST
            if p["mapped"] is not None:
                o["flags"] |= F_PORTMAP
                o["dport"] = p["mapped"]
            if p["rev"]:
                o["flags"] |= F_REV_PROXY
            tci[i] |= p["tc"]
            if r == TAILCALL:
                ep = p["ep"]
                o["stage"], o["lxc_id"] = STAGE_POLICY, ep["lxc_id"]
                sid[i], ifx[i], lid[i] = p["secctx"], ep["ifindex"], ep["lxc_id"]
                dl.append(i)
            elif r == ENCAP:                                 # redirect(ENCAP_IFINDEX) (encap.h:69)
                o["action"], o["ifindex_lo"], o["daddr4"] = TC_ACT_REDIRECT, self.encap_ifindex & 0xffff, p["tunnel"]
            elif r == ICMP6_TE:
                o["action"] = TC_ACT_REDIRECT
                o["flags"] |= F_ICMP6_TE
            elif r < 0:                                      # send_drop_notify_error(skb, ret, TC_ACT_SHOT) (:405-406, :446-447)
                o["action"], o["reason"] = TC_ACT_SHOT, -r
            else:
                o["action"] = r
        dl = np.array(dl, np.int64)
        f = lambda x: None if x is None else x[dl]
        sub = Packets(frames[dl].copy(), pk.lens[dl], sid[dl], ifx[dl], lid[dl], tci[dl], f(pk.flow_hash))
        return rec, frames, dl, sub


def complete(rec, dl, ing):
    """The front's records with handle_policy's fields for the delivered packets."""
    out = rec.copy()
    for name in ("action", "reason", "ct_ret", "proxy_port", "ifindex_lo"):
        out[name][dl] = ing[name]
    out["flags"][dl] = (rec["flags"][dl] & 0xF0) | ing["flags"]
    return out
