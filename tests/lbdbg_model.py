"""handle_policy with DEBUG and LB_DEBUG defined: the reverse NAT of ipv4_policy /
ipv6_policy and its cilium_dbg_lb messages, restated per packet from the reference's
call sites (carlanton/cilium 1.0.0-rc9) on top of tests/dbg_model.py — TEST
INFRASTRUCTURE ONLY.

dbg_model asserts the reverse NAT absent; this model adds it, with its four messages:

  bpf/lib/lb.h:85-89            cilium_dbg_lb is cilium_dbg with LB_DEBUG, else nothing;
  bpf/lib/dbg.h:134-233         cilium_dbg is empty without DEBUG: both options are needed
  bpf/bpf_lxc.c:909-918         ipv4_policy: ret == CT_REPLY && rev_nat_index && !loopback -> lb4_rev_nat
                                (REV_NAT_F_TUPLE_SADDR), after ct_lookup4 (:896), before
                                policy_can_access_ingress (:920)
  bpf/bpf_lxc.c:801-808         ipv6_policy: rev_nat_index != 0 (any ct_lookup6 result) -> lb6_rev_nat
                                (flags 0), after ct_lookup6 (:794), before policy_can_access_ingress (:810)
  bpf/lib/lb.h:524-538          lb4_rev_nat (DBG_LB4_REVERSE_NAT_LOOKUP :531, before the map lookup)
  bpf/lib/lb.h:447-512          __lb4_rev_nat (DBG_LB4_REVERSE_NAT :456, before any rewrite)
  bpf/lib/lb.h:304-316          lb6_rev_nat (DBG_LB6_REVERSE_NAT_LOOKUP :310)
  bpf/lib/lb.h:253-293          __lb6_rev_nat (DBG_LB6_REVERSE_NAT :264)
  bpf/lib/lb.h:217-251          reverse_map_l4_port; bpf/lib/l4.h:50-60 l4_modify_port

DBG_LB4_LOOPBACK_SNAT_REV (lb.h:487) cannot occur: the caller excludes ct_state.loopback.
Still not modelled (asserted absent): an IPv6 destination that carries a reverse-NAT index
(bpf_lxc.c:776-792) and LRU eviction.  The ingress call takes parsed columns and returns
verdict records, no frames: the rewrite is modelled by the checks that decide its verdict.
The model is anchored on the C oracle (which runs the reverse NAT) exactly as dbg_model is:
tests.test_lb_debug.run_anchored compares verdicts and final CT maps on every batch.
"""
import struct

from tests import dbg_model as M
from tests.ctoff_model import csum_offset, l4_csum_replace_ok, skb_store_ok

F_LB_DEBUG = 512                                                  # GF_LXC_F_LB_DEBUG
DROP_UNKNOWN_L4, DROP_CSUM_L4 = 142, 154                          # bpf/lib/common.h:236, 248
EFAULT = 14                                                       # skb_load_bytes' error, passed through


def _table(maps, name):
    m = maps.get(name) if name else None
    if m is None or m.keys is None:
        return {}
    return {bytes(k): bytes(v) for k, v in zip(m.keys, m.vals)}


class Program(M.Program):
    def __init__(self, e, maps, cts):
        super().__init__(e, maps, cts)
        self.revnat4 = _table(maps, e.get("revnat4"))             # cilium_lb4_reverse_nat: u16 -> {be32, be16}
        self.revnat6 = _table(maps, e.get("revnat6"))             # cilium_lb6_reverse_nat: u16 -> {v6addr, be16}


class LbDbgModel(M.DbgModel):
    def __init__(self, sc):
        super().__init__(sc)
        self.progs = {e["lxc_id"]: Program(e, sc.maps, self.ct) for e in sc.lxc}

    def _dbg_lb(self, p, name, a1, a2):
        """cilium_dbg_lb (lb.h:85-89): cilium_dbg under LB_DEBUG (and _dbg tests DEBUG)."""
        if p.flags & F_LB_DEBUG:
            self._dbg(p, name, a1, a2)

    def reverse_map_l4_port(self, nh, port, l4_off, l4w0, co):
        """lb.h:217-251.  The frame's source port is the first half of l4w0 (raw be16)."""
        if nh in (M.TCP, M.UDP):
            if port:
                if not (l4_off >= 0 and l4_off + 2 <= self.len):  # l4_load_port (:229-231)
                    return -EFAULT
                if port != (l4w0 & 0xffff):                       # l4_modify_port (l4.h:50-60)
                    if not l4_csum_replace_ok(l4_off + co, self.len):
                        return -DROP_CSUM_L4
                    if not skb_store_ok(l4_off, 2, self.len):
                        return -M.DROP_WRITE_ERROR
        elif nh not in (M.ICMP, M.ICMPV6):
            return -DROP_UNKNOWN_L4
        return 0

    def lb4_rev_nat(self, p, st, t, nh, l4_off, l4w0):
        """lb4_rev_nat + __lb4_rev_nat with REV_NAT_F_TUPLE_SADDR, ct_state->loopback == 0."""
        self._dbg_lb(p, "DBG_LB4_REVERSE_NAT_LOOKUP", st["rev_nat_index"], 0)           # lb.h:531
        nat = p.revnat4.get(struct.pack("<H", st["rev_nat_index"]))                      # :532
        if nat is None:
            return 0
        address, port = struct.unpack("<IH", nat)
        self._dbg_lb(p, "DBG_LB4_REVERSE_NAT", address, port)                            # lb.h:456
        co = csum_offset(nh)
        if port:                                                                         # :458-462
            r = self.reverse_map_l4_port(nh, port, l4_off, l4w0, co)
            if r < 0:
                return r
        t["saddr"] = nat[:4]                                                             # :464-466
        # (:499-505: the saddr store and l3_csum_replace lie inside the 34 B revalidate_data checked)
        if co and not l4_csum_replace_ok(l4_off + co, self.len):                         # :507-509
            return -DROP_CSUM_L4
        return 0

    def lb6_rev_nat(self, p, index, nh, l4_off, l4w0):
        """lb6_rev_nat + __lb6_rev_nat with flags 0 (the tuple is left alone)."""
        self._dbg_lb(p, "DBG_LB6_REVERSE_NAT_LOOKUP", index, 0)                          # lb.h:310
        nat = p.revnat6.get(struct.pack("<H", index))                                    # :311
        if nat is None:
            return 0
        p4, port = struct.unpack_from("<IH", nat, 12)
        self._dbg_lb(p, "DBG_LB6_REVERSE_NAT", p4, port)                                 # lb.h:264
        co = csum_offset(nh)
        if port:                                                                         # :266-270
            r = self.reverse_map_l4_port(nh, port, l4_off, l4w0, co)
            if r < 0:
                return r
        # (:277-286: ipv6_load_saddr / ipv6_store_saddr lie inside the 54 B checked)
        if not l4_csum_replace_ok(l4_off + co, self.len):                                # :288-290, unconditional
            return -DROP_CSUM_L4
        return 0

    def ip_policy(self, p, v6, saddr, daddr, nh, l4_off, l4w0, l4w3, src_label, ifindex, tc_index, now):
        """ipv4_policy / ipv6_policy as in dbg_model, with the reverse NAT between ct_lookup and the
        policy (bpf_lxc.c:801-808, 909-918) instead of the assertion that it does not occur."""
        if self.len < (54 if v6 else 34):
            return -M.DROP_INVALID, 0, ifindex, 0, 0
        t = {"daddr": daddr, "saddr": saddr, "dport": 0, "sport": 0, "nexthdr": nh, "flags": 0}
        if tc_index & 1:
            self._dbg(p, "DBG_SKIP_PROXY", tc_index, 0)
        skip_proxy = bool(tc_index & 1)
        rev_nat_new = 0
        if v6:
            rev_nat_new = daddr[12] | (daddr[13] << 8)
            assert not rev_nat_new, "not modelled"
        ct = p.ct6 if v6 else p.ct4
        st = {"rev_nat_index": 0, "loopback": 0}
        ret = self.ct_lookup(p, ct, v6, t, l4_off, l4w0, l4w3, st, now)
        if ret < 0:
            return ret, 0, ifindex, 0, 0
        reason = ret
        if v6:
            if st["rev_nat_index"]:                                                      # bpf_lxc.c:801
                ret2 = self.lb6_rev_nat(p, st["rev_nat_index"], nh, l4_off, l4w0)
                if ret2 < 0:
                    return ret2, reason, ifindex, 0, 0
        elif ret == M.CT_REPLY and st["rev_nat_index"] and not st["loopback"]:           # bpf_lxc.c:909-910
            ret2 = self.lb4_rev_nat(p, st, t, nh, l4_off, l4w0)
            if ret2 < 0:
                return ret2, reason, ifindex, 0, 0
        verdict = self.policy_can_access_ingress(p, src_label, t["dport"], nh, t["saddr"] if v6 else saddr)
        if ret not in (M.CT_REPLY, M.CT_RELATED) and verdict < 0:
            if ret == M.CT_ESTABLISHED:
                del ct.d[self._key(v6, t["daddr"], t["saddr"], t["dport"], t["sport"], nh, t["flags"])]
            return -M.DROP_POLICY, reason, ifindex, 0, 0
        if skip_proxy:
            verdict = 0
        flags = 0
        if ret == M.CT_NEW:
            ret = self.ct_create(p, ct, v6, t, rev_nat_new, src_label, now)
            if ret < 0:
                return ret, reason, ifindex, 0, 0
            flags |= M.ING_F_CREATED
        if verdict > 0 and ret in (M.CT_NEW, M.CT_ESTABLISHED):
            r = self.redirect(p, v6, l4_off, nh, verdict & 0xffff, t["dport"], daddr, t, src_label, reason, now)
            if r < 0:
                return r, reason, ifindex, flags, 0
            if not v6:
                self._dbg(p, "DBG_TO_HOST", 0, 0)
            return 0, reason, self.host_ifindex, flags | M.ING_F_PROXY, verdict & 0xffff
        return 0, reason, ifindex, flags, 0
