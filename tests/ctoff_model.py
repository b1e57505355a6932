"""handle_policy of an endpoint program compiled without CONNTRACK, restated per
packet from the reference (carlanton/cilium 1.0.0-rc9) — TEST INFRASTRUCTURE ONLY.

The CPU oracle cannot express the Conntrack endpoint option disabled
(pkg/endpoint/endpoint.go:111-114), so the tests own this model.  It follows the
reference line by line, not libgpuflow's kernels:

  bpf/lib/conntrack.h:582-617   !CONNTRACK: ct_lookup4/6 return 0 (CT_NEW) and touch
                                neither the map nor the tuple; ct_create4/6 return 0;
                                ct_delete4/6 are empty
  bpf/bpf_lxc.c:980-1024        handle_policy
  bpf/bpf_lxc.c:865-970         ipv4_policy
  bpf/bpf_lxc.c:745-862         ipv6_policy
  bpf/lib/policy.h:42-113       __policy_can_access
  bpf/lib/policy.h:133-191      policy_can_access_ingress
  bpf/lib/lxc.h:96-190          ipv{4,6}_redirect_to_host_port
  bpf/lib/l4.h:50-60            l4_modify_port
  bpf/lib/l4.h:138-139          CFG_L3L4_* refused without CONNTRACK (l4_proxy_lookup is 0)
  bpf/lib/csum.h:45-79          csum_l4_offset_and_flags, csum_l4_replace

Header fields come from the parsed columns (the skb_load_bytes / revalidate_data
rules of gf_parse_frames, checked against the oracle elsewhere): ethertype, raw
addresses, protocol / nexthdr after ipv6_hdrlen(), l4_off.  Kernel helper rules used:
bpf_l4_csum_replace fails for an offset > 0xffff, an odd offset or offset + 2 > len;
bpf_skb_store_bytes for an offset > 0xffff or offset + n > len (net/core/filter.c).
"""
import struct

import numpy as np

ING_OUT = np.dtype([("action", "u1"), ("reason", "u1"), ("ct_ret", "u1"), ("flags", "u1"),
                    ("proxy_port", "<u2"), ("ifindex_lo", "<u2")])

TC_ACT_OK, TC_ACT_SHOT, TC_ACT_REDIRECT = 0, 2, 7                 # bpf/include/linux/pkt_cls.h
DROP_POLICY, DROP_INVALID, DROP_UNKNOWN_L3 = 133, 134, 139        # bpf/lib/common.h:224-256 (as -DROP_*)
DROP_MISSED_TAIL_CALL, DROP_WRITE_ERROR, DROP_CSUM_L4 = 140, 141, 154
CT_NEW = 0                                                        # bpf/lib/common.h:310-315
F_DROP_ALL, F_POLICY_INGRESS, F_HAVE_L4_POLICY, F_LXC_IPV4, F_NO_CONNTRACK = 1, 2, 4, 16, 128   # include/gpuflow.h
ING_F_PROXY = 1
PROXY_DEFAULT_LIFETIME = 720                                      # bpf/lib/common.h:433
TC_INDEX_F_SKIP_PROXY = 1
IPPROTO_TCP, IPPROTO_UDP, IPPROTO_ICMPV6 = 6, 17, 58


def csum_offset(nexthdr):
    """csum_l4_offset_and_flags (csum.h:45-64): offset of the L4 checksum field, 0 = none."""
    return {IPPROTO_TCP: 16, IPPROTO_UDP: 6, IPPROTO_ICMPV6: 2}.get(nexthdr, 0)


def l4_csum_replace_ok(off, length):
    return 0 <= off <= 0xffff and not (off & 1) and off + 2 <= length


def skb_store_ok(off, n, length):
    return 0 <= off <= 0xffff and off + n <= length


def csum_add(a, b):
    """csum_add (include/net/checksum.h): 32-bit ones-complement add."""
    r = a + b
    return (r & 0xffffffff) + (r >> 32)


def csum_fold(x):
    x = (x & 0xffff) + (x >> 16)
    x = (x & 0xffff) + (x >> 16)
    return ~x & 0xffff


def l4_csum_replace_by_diff(frame, cap, off, diff, mangled_0):
    """bpf_l4_csum_replace with from == 0 (net/core/filter.c: inet_proto_csum_replace_by_diff;
    BPF_F_MARK_MANGLED_0: a zero UDP checksum is left alone, a zero result becomes 0xffff;
    BPF_F_PSEUDO_HDR only matters for CHECKSUM_COMPLETE / PARTIAL skbs).  The frame is a
    snap of cap bytes: a field outside it is not held."""
    if frame is None or off + 2 > cap:
        return
    old = int(frame[off]) | (int(frame[off + 1]) << 8)
    if mangled_0 and not old:
        return
    new = csum_fold(csum_add(diff, 0xffffffff ^ old))
    if mangled_0 and not new:
        new = 0xffff
    frame[off], frame[off + 1] = new & 0xff, new >> 8


def policy_key(identity, dport_raw, proto):
    """struct policy_key (common.h:184-190), ingress (egress bit 0)."""
    return struct.pack("<IHBB", identity, dport_raw, proto, 0)


class Program:
    """One endpoint's compile-time configuration (lxc_config.h) as the scenario gives it."""

    def __init__(self, e, maps):
        self.flags = e["flags"]
        assert self.flags & F_NO_CONNTRACK
        assert not e.get("l4"), "CFG_L3L4_INGRESS needs CONNTRACK (l4.h:138-139)"
        self.policy_name = e.get("policy")
        m = maps[self.policy_name]
        # policy map: key -> [proxy_port (raw be16), packets, bytes]; rest: the value's pad bytes as given
        self.policy = {}
        self.policy_raw = {}
        for k, v in zip(m.keys if m.keys is not None else [], m.vals if m.vals is not None else []):
            kb, vb = bytes(k), bytes(v)
            pp, = struct.unpack_from("<H", vb, 0)
            pk_, by = struct.unpack_from("<QQ", vb, 8)
            self.policy[kb] = [pp, pk_, by]
            self.policy_raw[kb] = vb
        self.cidr4 = self._lpm(maps, e.get("cidr4"), 4)
        self.cidr6 = self._lpm(maps, e.get("cidr6"), 16)

    @staticmethod
    def _lpm(maps, name, alen):
        if not name:                                   # CIDR{4,6}_INGRESS_MAP undefined: lookup is 0 (maps.h:177,190)
            return []
        m = maps[name]
        out = []
        for k in (m.keys if m.keys is not None else []):
            kb = bytes(k)
            plen, = struct.unpack_from("<I", kb, 0)
            out.append((plen, int.from_bytes(kb[4:4 + alen], "big")))
        return out

    def lpm_hit(self, table, addr_bytes):
        """LPM trie lookup with the full-length key (maps.h:195-198): any covering prefix."""
        bits = 8 * len(addr_bytes)
        a = int.from_bytes(addr_bytes, "big")
        for plen, net in table:
            if plen == 0 or (a >> (bits - plen)) == (net >> (bits - plen)):
                return True
        return False

    def policy_dump(self):
        """The policy map as a dump returns it (key -> 24-B value), counters included."""
        out = {}
        for k, (pp, pk_, by) in self.policy.items():
            v = bytearray(self.policy_raw[k])
            struct.pack_into("<QQ", v, 8, pk_ & (2 ** 64 - 1), by & (2 ** 64 - 1))
            out[k] = bytes(v)
        return out


class CtOffModel:
    """State across batches: each CT-off program's policy counters and the node's proxy maps."""

    def __init__(self, sc):
        self.sc = sc
        self.progs = {e["lxc_id"]: Program(e, sc.maps) for e in sc.lxc if e["flags"] & F_NO_CONNTRACK}
        self.host_ifindex = sc.host_ifindex
        nd = sc.node or {}
        self.has_proxy4, self.has_proxy6 = bool(nd.get("proxy4")), bool(nd.get("proxy6"))
        self.proxy4, self.proxy6 = {}, {}              # inserts, key bytes -> value bytes (last write wins)

    # __policy_can_access (policy.h:42-113) + policy_can_access_ingress (:133-191)
    def policy_can_access_ingress(self, p, identity, dport, proto, length, cidr_addr):
        if p.flags & F_DROP_ALL:                        # :138-139
            return -DROP_POLICY
        if not p.flags & F_POLICY_INGRESS:              # :170-190: no POLICY_INGRESS -> TC_ACT_OK
            return TC_ACT_OK

        def hit(key):
            ent = p.policy.get(key)
            if ent is not None:                         # :67-68, 79-80, 91-92
                ent[1] += 1
                ent[2] += length
            return ent

        if p.flags & F_HAVE_L4_POLICY:                  # :60-71
            ent = hit(policy_key(identity, dport, proto))
            if ent is not None:
                return ent[0] if ent[0] else 0          # :102-108, l4_proxy_lookup is 0 without CFG_L3L4
        if hit(policy_key(identity, 0, 0)) is not None:  # :74-82
            return TC_ACT_OK
        if p.flags & F_HAVE_L4_POLICY:                  # :84-95
            ent = hit(policy_key(0, dport, proto))
            if ent is not None:
                return ent[0] if ent[0] else 0
        # cb[CB_POLICY] was cleared by policy_clear_mark (:97-100)
        if identity < 256:                              # identity_is_reserved, :149-155
            if len(cidr_addr) == 16 and p.lpm_hit(p.cidr6, cidr_addr):
                return TC_ACT_OK
            if len(cidr_addr) == 4 and p.lpm_hit(p.cidr4, cidr_addr):
                return TC_ACT_OK
        return -DROP_POLICY

    # ipv{4,6}_redirect_to_host_port (lxc.h:96-190): 0 or -DROP_*
    def redirect_to_host_port(self, v6, l4_off, length, nexthdr, new_port, old_port, old_ip, tuple_daddr, tuple_sport,
                              identity, now):
        co = csum_offset(nexthdr)
        # l4_modify_port (l4.h:50-60); any failure is DROP_WRITE_ERROR (lxc.h:119-121, 171-172)
        if not l4_csum_replace_ok(l4_off + co, length) or not skb_store_ok(l4_off + 2, 2, length):
            return -DROP_WRITE_ERROR
        # daddr / checksum stores: inside the header revalidate_data already covered
        if v6:
            key = tuple_daddr + struct.pack("<HHBB", new_port, tuple_sport, nexthdr, 0)
            val = old_ip + struct.pack("<HHII", old_port, 0, identity, (now + PROXY_DEFAULT_LIFETIME) & 0xffffffff)
            if self.has_proxy6:
                self.proxy6[key] = val
        else:
            key = tuple_daddr + struct.pack("<HHBB", new_port, tuple_sport, nexthdr, 0)
            val = old_ip + struct.pack("<HHII", old_port, 0, identity, (now + PROXY_DEFAULT_LIFETIME) & 0xffffffff)
            if self.has_proxy4:
                self.proxy4[key] = val
        return 0

    def packet(self, p, ethertype, length, saddr4, daddr4, saddr6, daddr6, nexthdr, l4_off, src_label, ifindex, tc_index,
               now, frame=None):
        """handle_policy (bpf_lxc.c:980-1024).  Returns (record tuple, reached ipv{4,6}_policy).
        frame (optional, a writable uint8 snap of the skb): receives the program's header writes."""
        reached = False
        cb_ifindex = ifindex
        flags = proxy_port = 0
        if p.flags & F_DROP_ALL:                        # :986-989
            ret = -DROP_POLICY
        elif ethertype == 0x86DD:                       # :991-993
            reached = True
            ret, cb_ifindex, flags, proxy_port = self.ip_policy(p, True, length, saddr6, daddr6, nexthdr, l4_off,
                                                                 src_label, ifindex, tc_index, now, frame)
        elif ethertype == 0x0800 and p.flags & F_LXC_IPV4:   # :995-999
            reached = True
            ret, cb_ifindex, flags, proxy_port = self.ip_policy(p, False, length, saddr4, daddr4, nexthdr, l4_off,
                                                                 src_label, ifindex, tc_index, now)
        else:
            ret = -DROP_UNKNOWN_L3                      # :1001-1003
        if ret < 0:                                     # :1009-1011 send_drop_notify(..., TC_ACT_SHOT)
            return (TC_ACT_SHOT, -ret, CT_NEW, 0, 0, 0), reached
        # :1018-1023
        return (TC_ACT_REDIRECT if cb_ifindex else TC_ACT_OK, 0, CT_NEW, flags, proxy_port, cb_ifindex & 0xffff), reached

    def ip_policy(self, p, v6, length, saddr, daddr, nexthdr, l4_off, src_label, ifindex, tc_index, now, frame=None):
        """ipv4_policy (:865-970) / ipv6_policy (:745-862) with the stub ct_*.
        Returns (ret, cb[CB_IFINDEX], record flags, proxy port)."""
        if length < (54 if v6 else 34):                 # revalidate_data (:758, :878)
            return -DROP_INVALID, ifindex, 0, 0
        # tuple = {daddr, saddr, dport 0, sport 0, nexthdr, flags 0}: ct_lookup fills nothing (conntrack.h:583-595)
        skip_proxy = bool(tc_index & TC_INDEX_F_SKIP_PROXY)   # :770, :886
        if v6:
            rev_nat_index = daddr[12] | (daddr[13] << 8)      # ip6->daddr.s6_addr32[3] & 0xFFFF (:776)
            if rev_nat_index:                                 # :777-792 (the daddr store lies inside the header)
                cap = 0 if frame is None else min(length, len(frame))
                if frame is not None:                         # dip.p4 &= ~0xFFFF; ipv6_store_daddr (:780-782)
                    frame[38 + 12] = frame[38 + 13] = 0
                co = csum_offset(nexthdr)
                if co and not l4_csum_replace_ok(l4_off + co, length):
                    return -DROP_CSUM_L4, ifindex, 0, 0
                if co:                                        # :786-791: csum_diff(&rev_nat_index, 4, &zero, 4, 0)
                    diff = csum_add(0xffffffff ^ rev_nat_index, 0)
                    l4_csum_replace_by_diff(frame, cap, l4_off + co, diff, nexthdr == IPPROTO_UDP)
        # ret = ct_lookup{4,6}() = 0 = CT_NEW (:794, :896); ct_state stays zero: no rev-NAT (:801, :909)
        verdict = self.policy_can_access_ingress(p, src_label, 0, nexthdr, length, saddr)   # :810-812, :920-922
        if verdict < 0:                                 # :816-823, :926-933 (ret is neither REPLY nor RELATED)
            return -DROP_POLICY, ifindex, 0, 0
        if skip_proxy:                                  # :825-826, :935-936
            verdict = 0
        # ct_create{4,6}() = 0: ret stays CT_NEW (:828-836, :938-946)
        if verdict > 0:                                 # redirect_to_proxy(verdict) && ret == CT_NEW (:838, :948)
            r = self.redirect_to_host_port(v6, l4_off, length, nexthdr, verdict & 0xffff, 0, daddr, daddr, 0,
                                           src_label, now)
            if r < 0:
                return r, ifindex, 0, 0
            return 0, self.host_ifindex, ING_F_PROXY, verdict & 0xffff   # :858, :966
        return 0, ifindex, 0, 0

    def batch(self, pk, cols, now, mask=None, write_frames=False):
        """Runs the packets of CT-off programs (optionally only those in mask) in batch
        order.  Returns (indices, records ING_OUT, reached bool array).  write_frames:
        pk.frames receive the programs' header writes (the pipeline's snaps)."""
        idx, recs, reached = [], [], []
        lid = pk.lxc_id
        for i in range(pk.n):
            if mask is not None and not mask[i]:
                continue
            p = self.progs.get(int(lid[i]))
            if p is None:
                continue
            rec, rch = self.packet(
                p, int(cols["ethertype"][i]), int(pk.lens[i]), cols["saddr4"][i:i + 1].astype("<u4").tobytes(),
                cols["daddr4"][i:i + 1].astype("<u4").tobytes(), bytes(cols["saddr6"][i]), bytes(cols["daddr6"][i]),
                int(cols["proto"][i]), int(cols["l4_off"][i]), int(pk.src_identity[i]) if pk.src_identity is not None else 0,
                int(pk.ifindex[i]) if pk.ifindex is not None else 0, int(pk.tc_index[i]) if pk.tc_index is not None else 0,
                now, pk.frames[i] if write_frames else None)
            idx.append(i)
            recs.append(rec)
            reached.append(rch)
        out = np.zeros(len(recs), ING_OUT)
        for j, r in enumerate(recs):
            out[j] = r
        return np.array(idx, np.int64), out, np.array(reached, bool)


WORLD_ID = 2                                                      # bpf/lib/common.h (reserved identity "world")


def netdev_inputs(sc, frames, stage_policy):
    """What bpf_netdev hands to handle_policy for the frames it tail-calls into
    cilium_policy (stage_policy: bool per frame), from the frames as they are at that
    point: (cb[CB_SRC_LABEL], cb[CB_IFINDEX], lxc_id).
      bpf_netdev.c:50-64    derive_sec_ctx: FIXED_SRC_SECCTX, else the flow label when the
                            source lies in ROUTER_IP/64, else WORLD_ID
      bpf_netdev.c:249-261  derive_ipv4_sec_ctx: FIXED_SRC_SECCTX, else WORLD_ID
      bpf_netdev.c:216-222, 345-352  lookup_ip{4,6}_endpoint(daddr) in cilium_lxc
      bpf/lib/l3.h:129-130, 159-163  cb[CB_SRC_LABEL] = seclabel, cb[CB_IFINDEX] = ep->ifindex,
                            tail_call(cilium_policy, ep->lxc_id)"""
    nd = sc.netdev
    fixed = nd.get("fixed_secctx", 0) if nd.get("flags", 0) & 1 else None
    router = bytes(nd.get("router_ip6", bytes(16)))[:8]
    lxc = sc.maps[nd["lxc_map"]]
    eps = {bytes(k): (struct.unpack_from("<I", bytes(v), 0)[0], struct.unpack_from("<H", bytes(v), 6)[0])
           for k, v in zip(lxc.keys, lxc.vals)}
    n = len(frames)
    sid, ifx, lid = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.uint16)
    for i in np.nonzero(stage_policy)[0]:
        f = frames[i]
        if f[12] == 0x86 and f[13] == 0xDD:
            key = bytes(f[38:54]) + bytes([2, 0, 0, 0])           # endpoint_key, ENDPOINT_KEY_IPV6
            if fixed is not None:
                sid[i] = fixed
            elif bytes(f[22:30]) == router:
                sid[i] = ((int(f[15]) & 0x0f) << 16) | (int(f[16]) << 8) | int(f[17])   # IPV6_FLOWLABEL_MASK
            else:
                sid[i] = WORLD_ID
        else:
            key = bytes(f[30:34]) + bytes(12) + bytes([1, 0, 0, 0])   # ENDPOINT_KEY_IPV4
            sid[i] = fixed if fixed is not None else WORLD_ID
        ifx[i], lid[i] = eps[key]
    return sid, ifx, lid
