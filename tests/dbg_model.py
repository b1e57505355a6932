"""handle_policy with DEBUG defined, restated per packet from the reference's call
sites (carlanton/cilium 1.0.0-rc9) — TEST INFRASTRUCTURE ONLY.

The CPU oracle knows nothing about cilium_dbg*, so the tests own this model.  It is
written from the reference, not from libgpuflow's kernels, over dict CT / policy /
proxy maps, and returns per packet the verdict tuple and the ordered list of
notifications (debug, trace and drop records, as cilium_amd.monitor decodes them):

  bpf/bpf_lxc.c:980-1024        handle_policy (send_drop_notify / TRACE_TO_LXC last)
  bpf/bpf_lxc.c:865-970         ipv4_policy (DBG_TO_HOST :958)
  bpf/bpf_lxc.c:745-862         ipv6_policy
  bpf/lib/lxc.h:196-205         tc_index_skip_proxy (DBG_SKIP_PROXY)
  bpf/lib/conntrack.h:75-135    __ct_lookup (DBG_CT_MATCH :84)
  bpf/lib/conntrack.h:165-289   ct_lookup6 (DBG_CT_LOOKUP6_1/_2 :265-267, DBG_CT_VERDICT :287)
  bpf/lib/conntrack.h:319-435   ct_lookup4 (DBG_CT_LOOKUP4_1/_2 :413-415, DBG_CT_VERDICT :433)
  bpf/lib/conntrack.h:446-580   ct_create6 / ct_create4 (DBG_CT_CREATED6 :465, DBG_CT_CREATED4 :527)
  bpf/lib/policy.h:42-168       __policy_can_access (DBG_L4_CREATE :63), policy_can_access_ingress
                                (DBG_POLICY_DENIED :157)
  bpf/lib/l4.h:151-216          l4_proxy_lookup (DBG_GENERIC :198, DBG_L4_POLICY :203)
  bpf/lib/lxc.h:96-190          ipv{4,6}_redirect_to_host_port (TRACE_TO_PROXY :116/:168,
                                DBG_CAPTURE_PROXY_POST :133/:184, DBG_REV_PROXY_UPDATE :135)

Not modelled (asserted absent): rev-NAT (ct_state.rev_nat_index != 0 needs lb{4,6}_rev_nat)
and LRU eviction.  ct_delete4/6's DBG_ERROR_RET cannot occur: the tuple deleted is the one
just matched.  Column batches carry no frames: captures are zeros.
"""
import struct

import numpy as np

from cilium_amd import monitor as MON
from tests.ctoff_model import (ING_OUT, Program as _PolicyProgram, csum_offset, l4_csum_replace_ok, policy_key,
                               skb_store_ok)

TC_ACT_OK, TC_ACT_SHOT, TC_ACT_REDIRECT = 0, 2, 7
DROP_POLICY, DROP_INVALID, DROP_CT_INVALID_HDR, DROP_CT_UNKNOWN_PROTO = 133, 134, 135, 137
DROP_UNKNOWN_L3, DROP_MISSED_TAIL_CALL, DROP_WRITE_ERROR = 139, 140, 141
DROP_CT_CREATE_FAILED, DROP_PROXYMAP_CREATE_FAILED = 155, 161
CT_NEW, CT_ESTABLISHED, CT_REPLY, CT_RELATED = 0, 1, 2, 3
CT_INGRESS = 1
CT_DEFAULT_LIFETIME, CT_SYN_TIMEOUT, CT_CLOSE_TIMEOUT = 43200, 300, 10
PROXY_DEFAULT_LIFETIME = 720
TUPLE_F_OUT, TUPLE_F_IN, TUPLE_F_RELATED = 0, 1, 2
ACTION_UNSPEC, ACTION_CREATE, ACTION_CLOSE = 0, 1, 2
F_DROP_ALL, F_POLICY_INGRESS, F_HAVE_L4_POLICY, F_CT_ACCOUNTING, F_LXC_IPV4 = 1, 2, 4, 8, 16
F_TRACE_NOTIFY, F_NO_CONNTRACK, F_DEBUG = 64, 128, 256
ING_F_PROXY, ING_F_CREATED = 1, 2
TCP, UDP, ICMP, ICMPV6 = 6, 17, 1, 58
HASH = 1
TRACE_PAYLOAD_LEN = 128


def ntohs(x):
    return ((x & 0xff) << 8) | (x >> 8)


class Entry:
    """struct ct_entry (common.h)."""
    __slots__ = ("rx_packets", "rx_bytes", "tx_packets", "tx_bytes", "lifetime", "rx_closing", "tx_closing", "nat46",
                 "lb_loopback", "seen_non_syn", "rev_nat_index", "unused", "src_sec_id")

    def __init__(self, raw=None):
        if raw is None:
            raw = bytes(48)
        self.rx_packets, self.rx_bytes, self.tx_packets, self.tx_bytes, self.lifetime, fl, self.rev_nat_index, \
            self.unused, _pad, self.src_sec_id = struct.unpack("<QQQQIHHHHI", raw)
        self.rx_closing, self.tx_closing, self.nat46 = fl & 1, (fl >> 1) & 1, (fl >> 2) & 1
        self.lb_loopback, self.seen_non_syn = (fl >> 3) & 1, (fl >> 4) & 1

    def raw(self):
        fl = self.rx_closing | self.tx_closing << 1 | self.nat46 << 2 | self.lb_loopback << 3 | self.seen_non_syn << 4
        return struct.pack("<QQQQIHHHHI", self.rx_packets, self.rx_bytes, self.tx_packets, self.tx_bytes,
                           self.lifetime & 0xffffffff, fl, self.rev_nat_index, self.unused, 0, self.src_sec_id)

    def copy(self):
        return Entry(self.raw())


class CtMap:
    def __init__(self, spec):
        self.type, self.max_entries = spec.type, spec.max_entries
        self.d = {}
        for k, v in zip(spec.keys if spec.keys is not None else [], spec.vals if spec.vals is not None else []):
            self.d[bytes(k)] = Entry(bytes(v))

    def update(self, key, entry):
        """map_update_elem(BPF_ANY): a HASH map at max_entries refuses a new key (E2BIG)."""
        if key not in self.d and self.type == HASH and len(self.d) >= self.max_entries:
            return -1
        self.d[key] = entry.copy()
        return 0

    def dump(self):
        return {k: e.raw() for k, e in self.d.items()}


class Program(_PolicyProgram):
    def __init__(self, e, maps, cts):
        self.flags = e["flags"]
        assert not self.flags & F_NO_CONNTRACK
        self.lxc_id, self.seclabel = e["lxc_id"], e["seclabel"]
        self.l4 = [(ntohs(p), ntohs(x), nh) for p, x, nh in (e.get("l4") or [])]     # raw be16 port, proxy
        self.ct4, self.ct6 = cts.get(e.get("ct4")), cts.get(e.get("ct6"))
        self.policy, self.policy_raw = {}, {}
        m = maps[e["policy"]]
        for k, v in zip(m.keys if m.keys is not None else [], m.vals if m.vals is not None else []):
            kb, vb = bytes(k), bytes(v)
            self.policy[kb] = [struct.unpack_from("<H", vb, 0)[0], *struct.unpack_from("<QQ", vb, 8)]
            self.policy_raw[kb] = vb
        self.cidr4 = self._lpm(maps, e.get("cidr4"), 4)
        self.cidr6 = self._lpm(maps, e.get("cidr6"), 16)


class DbgModel:
    def __init__(self, sc):
        self.sc = sc
        names = {e.get(f) for e in sc.lxc for f in ("ct4", "ct6")} - {None}
        self.ct = {n: CtMap(sc.maps[n]) for n in names}
        self.progs = {e["lxc_id"]: Program(e, sc.maps, self.ct) for e in sc.lxc}
        nd = sc.node or {}
        self.px = {4: nd.get("proxy4"), 6: nd.get("proxy6")}
        self.proxy = {4: {}, 6: {}}
        self.px_max = {f: sc.maps[n].max_entries for f, n in self.px.items() if n}
        self.host_ifindex = sc.host_ifindex

    # ---- notifications -------------------------------------------------------------------------------
    def _dbg(self, p, name, a1, a2, a3=0):
        """cilium_dbg / cilium_dbg3 (dbg.h:151-181); EVENT_SOURCE = LXC_ID."""
        if p.flags & F_DEBUG:
            self.ev.append(dict(type=MON.NOTIFY_DBG_MSG, subtype=MON.DBG_NAMES.index(name), source=p.lxc_id, hash=self.hash,
                                name=name, arg1=a1 & 0xffffffff, arg2=a2 & 0xffffffff, arg3=a3 & 0xffffffff))

    def _capture(self, p, name, a1):
        """cilium_dbg_capture (dbg.h:191-214)."""
        if p.flags & F_DEBUG:
            cap = min(TRACE_PAYLOAD_LEN, self.len)
            self.ev.append(dict(type=MON.NOTIFY_DBG_CAPTURE, subtype=MON.DBG_CAPTURE_NAMES.index(name), source=p.lxc_id,
                                hash=self.hash, name=name, len_orig=self.len, len_cap=cap, arg1=a1, arg2=0,
                                data=bytes(cap)))

    def _trace(self, p, obs, src, dst, dst_id, ifindex, reason):
        """send_trace_notify (trace.h:73-106)."""
        if p.flags & F_TRACE_NOTIFY:
            cap = min(TRACE_PAYLOAD_LEN, self.len)
            self.ev.append(dict(type=MON.NOTIFY_TRACE, subtype=obs, source=p.lxc_id, hash=self.hash,
                                name=MON.TRACE_NAMES[obs], len_orig=self.len, len_cap=cap, src_label=src, dst_label=dst,
                                dst_id=dst_id & 0xffff, reason=reason & 0xff, ifindex=ifindex, data=bytes(cap)))

    def _drop(self, source, reason, src, dst, dst_id, ifindex):
        """send_drop_notify (drop.h:47-107): labels are u16 in the tail-call metadata."""
        cap = min(TRACE_PAYLOAD_LEN, self.len)
        self.ev.append(dict(type=MON.NOTIFY_DROP, subtype=reason, source=source & 0xffff, hash=self.hash, reason=reason,
                            len_orig=self.len, len_cap=cap, src_label=src & 0xffff, dst_label=dst & 0xffff, dst_id=dst_id,
                            ifindex=ifindex, data=bytes(cap)))

    # ---- conntrack -----------------------------------------------------------------------------------
    def _ct_lookup_one(self, p, ct, key, action, st, syn, now):
        """__ct_lookup (conntrack.h:75-135), dir = CT_INGRESS."""
        e = ct.d.get(key)
        if e is None:
            return CT_NEW
        self._dbg(p, "DBG_CT_MATCH", e.lifetime, e.rev_nat_index)
        if not e.rx_closing or not e.tx_closing:                  # ct_entry_alive -> ct_update_timeout
            self._timeout(e, syn, now)
        st["rev_nat_index"], st["loopback"] = e.rev_nat_index, e.lb_loopback
        if p.flags & F_CT_ACCOUNTING:
            e.rx_packets += 1
            e.rx_bytes += self.len
        if action == ACTION_CREATE:
            if e.rx_closing + e.tx_closing >= 1:
                e.rx_closing = e.tx_closing = 0
                self._timeout(e, syn, now)
        elif action == ACTION_CLOSE:
            e.rx_closing = 1
            if not (not e.rx_closing or not e.tx_closing):
                e.lifetime = now + CT_CLOSE_TIMEOUT
        return CT_ESTABLISHED

    @staticmethod
    def _timeout(e, syn, now):
        e.seen_non_syn |= int(not syn)
        e.lifetime = now + (CT_DEFAULT_LIFETIME if e.seen_non_syn else CT_SYN_TIMEOUT)

    @staticmethod
    def _key(v6, daddr, saddr, dport, sport, nh, flags):
        return daddr + saddr + struct.pack("<HHBB", dport, sport, nh, flags) + (b"\0\0" if v6 else b"")

    def ct_lookup(self, p, ct, v6, t, l4_off, l4w0, l4w3, st, now):
        """ct_lookup4 / ct_lookup6, dir = CT_INGRESS.  t: dict tuple, changed in place."""
        action, syn = ACTION_UNSPEC, False
        t["flags"] = TUPLE_F_OUT
        nh = t["nexthdr"]
        ld = lambda off, n: off >= 0 and off + n <= self.len   # skb_load_bytes
        if nh == (ICMPV6 if v6 else ICMP):
            if not ld(l4_off, 1):
                return -DROP_CT_INVALID_HDR
            typ = l4w0 & 0xff
            t["sport"] = t["dport"] = 0
            related, reply, request = ((1, 2, 3, 4), 129, 128) if v6 else ((3, 11, 12), 0, 8)
            if typ in related:
                t["flags"] |= TUPLE_F_RELATED
            elif typ == reply:
                t["dport"] = request
            else:
                if typ == request:
                    t["sport"] = typ
                action = ACTION_CREATE
        elif nh == TCP:
            if not ld(l4_off + 12, 2):
                return -DROP_CT_INVALID_HDR
            fin, sy, rst = (l4w3 >> 8) & 1, (l4w3 >> 9) & 1, (l4w3 >> 10) & 1
            action = ACTION_CLOSE if (rst or fin) else ACTION_CREATE
            syn = bool(sy)
            if not ld(l4_off, 4):
                return -DROP_CT_INVALID_HDR
            t["dport"], t["sport"] = l4w0 & 0xffff, l4w0 >> 16       # 4 bytes at &tuple->dport
        elif nh == UDP:
            if not ld(l4_off, 4):
                return -DROP_CT_INVALID_HDR
            t["dport"], t["sport"] = l4w0 & 0xffff, l4w0 >> 16
            action = ACTION_CREATE
        else:
            return -DROP_CT_UNKNOWN_PROTO
        ports = (ntohs(t["sport"]) << 16) | ntohs(t["dport"])
        if v6:
            self._dbg(p, "DBG_CT_LOOKUP6_1", int.from_bytes(t["saddr"][12:], "little"),
                      int.from_bytes(t["daddr"][12:], "little"), ports)
            self._dbg(p, "DBG_CT_LOOKUP6_2", (nh << 8) | t["flags"], 0, 0)
        else:
            self._dbg(p, "DBG_CT_LOOKUP4_1", int.from_bytes(t["saddr"], "little"), int.from_bytes(t["daddr"], "little"),
                      ports)
            self._dbg(p, "DBG_CT_LOOKUP4_2", (nh << 8) | t["flags"], 0, 0)
        ret = self._ct_lookup_one(p, ct, self._key(v6, t["daddr"], t["saddr"], t["dport"], t["sport"], nh, t["flags"]),
                                  action, st, syn, now)
        if ret != CT_NEW:
            ret = CT_RELATED if t["flags"] & TUPLE_F_RELATED else CT_REPLY
        else:
            t["saddr"], t["daddr"] = t["daddr"], t["saddr"]           # ipv{4,6}_ct_tuple_reverse
            t["sport"], t["dport"] = t["dport"], t["sport"]
            t["flags"] ^= TUPLE_F_IN
            ret = self._ct_lookup_one(p, ct, self._key(v6, t["daddr"], t["saddr"], t["dport"], t["sport"], nh, t["flags"]),
                                      action, st, syn, now)
        self._dbg(p, "DBG_CT_VERDICT", -ret if ret < 0 else ret, st["rev_nat_index"])
        return ret

    def ct_create(self, p, ct, v6, t, rev_nat_index, src_sec_id, now):
        """ct_create4 / ct_create6, dir = CT_INGRESS, ct_state->addr == 0."""
        e = Entry()
        e.rev_nat_index = rev_nat_index
        self._timeout(e, t["nexthdr"] == TCP, now)
        e.rx_packets, e.rx_bytes = 1, self.len
        if v6:
            self._dbg(p, "DBG_CT_CREATED6", e.rev_nat_index, src_sec_id, 0)
        else:
            self._dbg(p, "DBG_CT_CREATED4", e.rev_nat_index, src_sec_id, 0)
        e.src_sec_id = src_sec_id
        nh = t["nexthdr"]
        if ct.update(self._key(v6, t["daddr"], t["saddr"], t["dport"], t["sport"], nh, t["flags"]), e) < 0:
            return -DROP_CT_CREATE_FAILED
        e.seen_non_syn = 1
        if ct.update(self._key(v6, t["daddr"], t["saddr"], 0, 0, ICMPV6 if v6 else ICMP, t["flags"] | TUPLE_F_RELATED),
                     e) < 0:
            return -DROP_CT_CREATE_FAILED
        return 0

    # ---- policy --------------------------------------------------------------------------------------
    def l4_proxy_lookup(self, p, nh, dport):
        """l4_proxy_lookup(dir = CT_INGRESS) + BPF_L4_MAP (l4.h:151-216, common.h:105-127)."""
        proxy_port = 0
        if nh in (UDP, TCP):
            self._dbg(p, "DBG_GENERIC", dport, nh)
            for port, proxy, proto in p.l4:
                if port and port == dport and proto and proto == nh:
                    proxy_port = proxy
                    break
            self._dbg(p, "DBG_L4_POLICY", proxy_port, CT_INGRESS)
        return proxy_port

    def policy_can_access_ingress(self, p, identity, dport, proto, cidr_addr):
        if not p.flags & F_POLICY_INGRESS:                        # policy.h:170-190
            return TC_ACT_OK

        def hit(key):
            ent = p.policy.get(key)
            if ent is not None:
                ent[1] += 1
                ent[2] += self.len
            return ent

        ent = None
        if p.flags & F_HAVE_L4_POLICY:                            # :60-71
            ent = hit(policy_key(identity, dport, proto))
            if ent is not None:
                self._dbg(p, "DBG_L4_CREATE", identity, p.seclabel, dport << 16 | proto)
        if ent is None:
            if hit(policy_key(identity, 0, 0)) is not None:       # :74-82
                return TC_ACT_OK
            if p.flags & F_HAVE_L4_POLICY:                        # :84-95
                ent = hit(policy_key(0, dport, proto))
        if ent is not None:                                       # get_proxy_port, :102-108
            return ent[0] if ent[0] else self.l4_proxy_lookup(p, proto, dport)
        if identity < 256:                                        # :149-155
            if len(cidr_addr) == 16 and p.lpm_hit(p.cidr6, cidr_addr):
                return TC_ACT_OK
            if len(cidr_addr) == 4 and p.lpm_hit(p.cidr4, cidr_addr):
                return TC_ACT_OK
        self._dbg(p, "DBG_POLICY_DENIED", identity, p.seclabel)   # :157
        return -DROP_POLICY

    def redirect(self, p, v6, l4_off, nh, new_port, old_port, old_ip, t, identity, reason, now):
        """ipv{4,6}_redirect_to_host_port (lxc.h:96-190)."""
        self._trace(p, 1, p.seclabel, 0, 0, self.host_ifindex, reason)            # TRACE_TO_PROXY
        co = csum_offset(nh) if (v6 or nh != ICMPV6) else 0
        if not l4_csum_replace_ok(l4_off + co, self.len) or not skb_store_ok(l4_off + 2, 2, self.len):
            return -DROP_WRITE_ERROR
        self._capture(p, "DBG_CAPTURE_PROXY_POST", new_port)
        if not v6:
            self._dbg(p, "DBG_REV_PROXY_UPDATE", t["sport"] << 16 | new_port, int.from_bytes(t["daddr"], "little"), nh)
        fam = 6 if v6 else 4
        if self.px[fam]:
            key = t["daddr"] + struct.pack("<HHBB", new_port, t["sport"], nh, 0)
            val = old_ip + struct.pack("<HHII", old_port, 0, identity, (now + PROXY_DEFAULT_LIFETIME) & 0xffffffff)
            if key not in self.proxy[fam] and len(self.proxy[fam]) >= self.px_max[fam]:
                return -DROP_PROXYMAP_CREATE_FAILED
            self.proxy[fam][key] = val
        return 0

    def ip_policy(self, p, v6, saddr, daddr, nh, l4_off, l4w0, l4w3, src_label, ifindex, tc_index, now):
        """ipv4_policy / ipv6_policy.  Returns (ret, forwarding_reason, cb[CB_IFINDEX], flags, proxy_port)."""
        if self.len < (54 if v6 else 34):                         # revalidate_data
            return -DROP_INVALID, 0, ifindex, 0, 0
        t = {"daddr": daddr, "saddr": saddr, "dport": 0, "sport": 0, "nexthdr": nh, "flags": 0}
        if tc_index & 1:                                          # tc_index_skip_proxy
            self._dbg(p, "DBG_SKIP_PROXY", tc_index, 0)
        skip_proxy = bool(tc_index & 1)
        rev_nat_new = 0
        if v6:
            rev_nat_new = daddr[12] | (daddr[13] << 8)            # ip6->daddr.s6_addr32[3] & 0xFFFF
            assert not rev_nat_new, "not modelled"
        ct = p.ct6 if v6 else p.ct4
        st = {"rev_nat_index": 0, "loopback": 0}
        ret = self.ct_lookup(p, ct, v6, t, l4_off, l4w0, l4w3, st, now)
        if ret < 0:
            return ret, 0, ifindex, 0, 0
        reason = ret
        assert not st["rev_nat_index"], "rev-NAT is not modelled"
        verdict = self.policy_can_access_ingress(p, src_label, t["dport"], nh, t["saddr"] if v6 else saddr)
        if ret not in (CT_REPLY, CT_RELATED) and verdict < 0:
            if ret == CT_ESTABLISHED:                             # ct_delete4/6: the tuple just matched
                del ct.d[self._key(v6, t["daddr"], t["saddr"], t["dport"], t["sport"], nh, t["flags"])]
            return -DROP_POLICY, reason, ifindex, 0, 0
        if skip_proxy:
            verdict = 0
        flags = 0
        if ret == CT_NEW:
            ret = self.ct_create(p, ct, v6, t, rev_nat_new, src_label, now)
            if ret < 0:
                return ret, reason, ifindex, 0, 0
            flags |= ING_F_CREATED
        if verdict > 0 and ret in (CT_NEW, CT_ESTABLISHED):
            r = self.redirect(p, v6, l4_off, nh, verdict & 0xffff, t["dport"], daddr, t, src_label, reason, now)
            if r < 0:
                return r, reason, ifindex, flags, 0
            if not v6:
                self._dbg(p, "DBG_TO_HOST", 0, 0)                 # is_policy_skip: cb[CB_POLICY] was cleared
            return 0, reason, self.host_ifindex, flags | ING_F_PROXY, verdict & 0xffff
        return 0, reason, ifindex, flags, 0

    def packet(self, lxc_id, ethertype, length, saddr4, daddr4, saddr6, daddr6, nh, l4_off, l4w0, l4w3, src_label, ifindex,
               tc_index, flow_hash, now):
        """handle_policy.  Returns (record tuple, notifications)."""
        self.ev, self.len, self.hash = [], length, flow_hash
        p = self.progs.get(lxc_id)
        if p is None:                                             # missed tail call: the caller's drop notify
            self._drop(0, DROP_MISSED_TAIL_CALL, 0, 0, 0, 0)
            return (TC_ACT_SHOT, DROP_MISSED_TAIL_CALL, 0, 0, 0, 0), self.ev
        reason, cb_ifindex, flags, proxy = 0, ifindex, 0, 0
        if p.flags & F_DROP_ALL:
            ret = -DROP_POLICY
        elif ethertype == 0x86DD:
            ret, reason, cb_ifindex, flags, proxy = self.ip_policy(p, True, saddr6, daddr6, nh, l4_off, l4w0, l4w3,
                                                                   src_label, ifindex, tc_index, now)
        elif ethertype == 0x0800 and p.flags & F_LXC_IPV4:
            ret, reason, cb_ifindex, flags, proxy = self.ip_policy(p, False, saddr4, daddr4, nh, l4_off, l4w0, l4w3,
                                                                   src_label, ifindex, tc_index, now)
        else:
            ret = -DROP_UNKNOWN_L3
        if ret < 0:
            self._drop(p.lxc_id, -ret, src_label, p.seclabel, p.lxc_id, ifindex)
            return (TC_ACT_SHOT, -ret, reason, flags & ING_F_CREATED, 0, 0), self.ev
        if ifindex == cb_ifindex:
            self._trace(p, 0, src_label, p.seclabel, p.lxc_id, ifindex, reason)   # TRACE_TO_LXC
        return (TC_ACT_REDIRECT if cb_ifindex else TC_ACT_OK, 0, reason, flags, proxy, cb_ifindex & 0xffff), self.ev

    def batch(self, pk, cols, now):
        """The batch in order.  Returns (records ING_OUT, per-packet notification lists)."""
        out, evs = np.zeros(pk.n, ING_OUT), []
        opt = lambda a, i: int(a[i]) if a is not None else 0
        for i in range(pk.n):
            rec, ev = self.packet(opt(pk.lxc_id, i), int(cols["ethertype"][i]), int(pk.lens[i]),
                                  cols["saddr4"][i:i + 1].astype("<u4").tobytes(),
                                  cols["daddr4"][i:i + 1].astype("<u4").tobytes(), bytes(cols["saddr6"][i]),
                                  bytes(cols["daddr6"][i]), int(cols["proto"][i]), int(cols["l4_off"][i]),
                                  int(cols["l4w0"][i]), int(cols["l4w3"][i]), opt(pk.src_identity, i), opt(pk.ifindex, i),
                                  opt(pk.tc_index, i), opt(pk.flow_hash, i), now)
            out[i] = rec
            evs.append(ev)
        return out, evs
