"""Decoder for the records of the event ring (gf_set_event_ring): one
GF_EVENT_RECORD slot each, in the four layouts of the reference's
`cilium_events` perf ring as pkg/monitor decodes them —

  DropNotify    (datapath_drop.go,  bpf/lib/drop.h:38-46)   type 1, 32-B header
  DebugMsg      (datapath_debug.go, bpf/lib/dbg.h:144-149)  type 2, 20 B
  DebugCapture  (datapath_debug.go, bpf/lib/dbg.h:183-189)  type 3, 24-B header
  TraceNotify   (datapath_trace.go, bpf/lib/trace.h:59-71)  type 4, 32-B header

Headers with a capture are followed directly by len_cap frame bytes.
"""
import struct

import numpy as np

EVENT_RECORD = 160
NOTIFY_DROP, NOTIFY_DBG_MSG, NOTIFY_DBG_CAPTURE, NOTIFY_TRACE = 1, 2, 3, 4

# bpf/lib/dbg.h:22-110, in enum order (the subtype of a DebugMsg indexes this list)
DBG_NAMES = [
    "DBG_UNSPEC", "DBG_GENERIC", "DBG_LOCAL_DELIVERY", "DBG_ENCAP", "DBG_LXC_FOUND", "DBG_POLICY_DENIED",
    "DBG_CT_LOOKUP", "DBG_CT_LOOKUP_REV", "DBG_CT_MATCH", "DBG_CT_CREATED", "DBG_CT_CREATED2", "DBG_ICMP6_HANDLE",
    "DBG_ICMP6_REQUEST", "DBG_ICMP6_NS", "DBG_ICMP6_TIME_EXCEEDED", "DBG_CT_VERDICT", "DBG_DECAP", "DBG_PORT_MAP",
    "DBG_ERROR_RET", "DBG_TO_HOST", "DBG_TO_STACK", "DBG_PKT_HASH", "DBG_LB6_LOOKUP_MASTER",
    "DBG_LB6_LOOKUP_MASTER_FAIL", "DBG_LB6_LOOKUP_SLAVE", "DBG_LB6_LOOKUP_SLAVE_SUCCESS",
    "DBG_LB6_REVERSE_NAT_LOOKUP", "DBG_LB6_REVERSE_NAT", "DBG_LB4_LOOKUP_MASTER", "DBG_LB4_LOOKUP_MASTER_FAIL",
    "DBG_LB4_LOOKUP_SLAVE", "DBG_LB4_LOOKUP_SLAVE_SUCCESS", "DBG_LB4_REVERSE_NAT_LOOKUP", "DBG_LB4_REVERSE_NAT",
    "DBG_LB4_LOOPBACK_SNAT", "DBG_LB4_LOOPBACK_SNAT_REV", "DBG_CT_LOOKUP4", "DBG_RR_SLAVE_SEL",
    "DBG_REV_PROXY_LOOKUP", "DBG_REV_PROXY_FOUND", "DBG_REV_PROXY_UPDATE", "DBG_L4_POLICY", "DBG_NETDEV_IN_CLUSTER",
    "DBG_NETDEV_ENCAP4", "DBG_CT_LOOKUP4_1", "DBG_CT_LOOKUP4_2", "DBG_CT_CREATED4", "DBG_CT_LOOKUP6_1",
    "DBG_CT_LOOKUP6_2", "DBG_CT_CREATED6", "DBG_SKIP_PROXY", "DBG_L4_CREATE", "DBG_IP_ID_MAP_FAILED4",
    "DBG_IP_ID_MAP_FAILED6", "DBG_IP_ID_MAP_SUCCEED4", "DBG_IP_ID_MAP_SUCCEED6",
]
# bpf/lib/dbg.h:113-124
DBG_CAPTURE_NAMES = [
    "DBG_CAPTURE_UNSPEC", "DBG_CAPTURE_FROM_RESERVED1", "DBG_CAPTURE_FROM_RESERVED2", "DBG_CAPTURE_FROM_RESERVED3",
    "DBG_CAPTURE_DELIVERY", "DBG_CAPTURE_FROM_LB", "DBG_CAPTURE_AFTER_V46", "DBG_CAPTURE_AFTER_V64",
    "DBG_CAPTURE_PROXY_PRE", "DBG_CAPTURE_PROXY_POST",
]
# bpf/lib/trace.h:26-37
TRACE_NAMES = ["TRACE_TO_LXC", "TRACE_TO_PROXY", "TRACE_TO_HOST", "TRACE_TO_STACK", "TRACE_TO_OVERLAY",
               "TRACE_FROM_LXC", "TRACE_FROM_PROXY", "TRACE_FROM_HOST", "TRACE_FROM_STACK", "TRACE_FROM_OVERLAY"]


def _name(names, k):
    return names[k] if k < len(names) else str(k)


def decode(rec):
    """One ring slot (bytes or a uint8 array of EVENT_RECORD bytes) as a dict."""
    b = bytes(rec)
    t, sub, source, h = struct.unpack_from("<BBHI", b, 0)
    d = {"type": t, "subtype": sub, "source": source, "hash": h}
    if t == NOTIFY_DROP:
        lo, lc, s, dl, did, ifx = struct.unpack_from("<IIIIII", b, 8)
        d.update(reason=sub, len_orig=lo, len_cap=lc, src_label=s, dst_label=dl, dst_id=did, ifindex=ifx,
                 data=b[32:32 + lc])
    elif t == NOTIFY_TRACE:
        lo, lc, s, dl, did, reason, _pad, ifx = struct.unpack_from("<IIIIHBBI", b, 8)
        d.update(name=_name(TRACE_NAMES, sub), len_orig=lo, len_cap=lc, src_label=s, dst_label=dl, dst_id=did,
                 reason=reason, ifindex=ifx, data=b[32:32 + lc])
    elif t == NOTIFY_DBG_MSG:
        a1, a2, a3 = struct.unpack_from("<III", b, 8)
        d.update(name=_name(DBG_NAMES, sub), arg1=a1, arg2=a2, arg3=a3)
    elif t == NOTIFY_DBG_CAPTURE:
        lo, lc, a1, a2 = struct.unpack_from("<IIII", b, 8)
        d.update(name=_name(DBG_CAPTURE_NAMES, sub), len_orig=lo, len_cap=lc, arg1=a1, arg2=a2, data=b[24:24 + lc])
    return d


def _ntohs(x):
    return ((x & 0xff) << 8) | ((x >> 8) & 0xff)


def _ip4(x):
    return ".".join(str((x >> s) & 0xff) for s in (0, 8, 16, 24))      # a be32 as loaded on a little-endian host


def dbg_text(d):
    """The message part of DebugMsg.Dump (pkg/monitor/datapath_debug.go:279-302) for a decoded
    type-2 record of one of the load balancer's reverse-NAT subtypes (LB_DEBUG); for every
    other record, its subtype name."""
    name = d.get("name", str(d.get("subtype")))
    if d.get("type") != NOTIFY_DBG_MSG:
        return name
    a1, a2 = d["arg1"], d["arg2"]
    if name in ("DBG_LB6_REVERSE_NAT_LOOKUP", "DBG_LB4_REVERSE_NAT_LOOKUP"):
        return "Reverse NAT lookup, index=%d" % _ntohs(a1 & 0xffff)
    if name == "DBG_LB6_REVERSE_NAT":
        return "Performing reverse NAT, address.p4=%x port=%d" % (a1, _ntohs(a2 & 0xffff))
    if name == "DBG_LB4_REVERSE_NAT":
        return "Performing reverse NAT, address=%s port=%d" % (_ip4(a1), _ntohs(a2 & 0xffff))
    return name


def decode_ring(records, count=None):
    """The first `count` slots of a ring (a [capacity, EVENT_RECORD] uint8 array) as dicts."""
    a = np.asarray(records, np.uint8).reshape(-1, EVENT_RECORD)
    n = len(a) if count is None else min(int(count), len(a))
    return [decode(a[k]) for k in range(n)]


# ---- cilium monitor's filters (cilium/cmd/monitor.go:108-156) ----
def endpoints(rec):
    """(type, source, destination) as the four handlers of cilium/cmd/monitor.go pass them to
    match (:165,182,199,215): the destination is uint16(DstID) of a drop record, DstID of a trace
    record and 0 of a debug message or capture.  `rec` is a slot (bytes, uint8 array) or a dict of
    decode()."""
    if isinstance(rec, dict):
        t, src = rec["type"], rec["source"]
        dst = rec.get("dst_id", 0) & 0xffff if t in (NOTIFY_DROP, NOTIFY_TRACE) else 0
        return t, src, dst
    b = bytes(rec[:28])
    t, _sub, src = struct.unpack_from("<BBH", b, 0)
    dst = struct.unpack_from("<H", b, 24)[0] if t in (NOTIFY_DROP, NOTIFY_TRACE) else 0
    return t, src, dst


def match(rec, types=(), frm=(), to=(), related=()):
    """match() of cilium/cmd/monitor.go:144-156 over one record: an empty list is a flag that
    was not given.  A record of a type other than 1..4 never matches (the reference prints
    "Unknown event" for it whatever the filter)."""
    t, src, dst = endpoints(rec)
    if not NOTIFY_DROP <= t <= NOTIFY_TRACE:
        return False
    if len(types) and t not in types:
        return False
    if len(frm) and src not in frm:
        return False
    if len(to) and dst not in to:
        return False
    if len(related) and src not in related and dst not in related:
        return False
    return True


class EventFilter:
    """A gf_event_filter_load handle: `cilium monitor --type --from --to --related-to` for
    gf_event_drain (Datapath.event_drain).  types: message types 1..4; frm / to / related:
    endpoint ids (u16)."""

    def __init__(self, types=(), frm=(), to=(), related=()):
        import ctypes as C
        from ._lib import lib, gf_event_filter_cfg
        self.types, self.frm, self.to, self.related = tuple(types), tuple(frm), tuple(to), tuple(related)
        mask = 0
        for t in self.types:
            mask |= 1 << t
        lists = [(C.c_uint16 * max(len(x), 1))(*x) for x in (self.frm, self.to, self.related)]
        cfg = gf_event_filter_cfg(mask, lists[0], len(self.frm), lists[1], len(self.to), lists[2], len(self.related))
        self._lib = lib
        self.handle = lib.gf_event_filter_load(C.byref(cfg))
        if self.handle < 0:
            raise OSError(-self.handle, "gf_event_filter_load")

    def match(self, rec):
        return match(rec, self.types, self.frm, self.to, self.related)

    def close(self):
        if self.handle > 0:
            self._lib.gf_obj_close(self.handle)
            self.handle = 0


def decode_packed(buf, offsets):
    """The records of a packed drain (GF_EVD_F_PACKED) as dicts: `offsets` holds the byte offset
    of every record and the total, as gf_event_drain's out_off does."""
    a = np.asarray(buf, np.uint8).reshape(-1)
    off = [int(x) for x in offsets]
    out = []
    for lo, hi in zip(off[:-1], off[1:]):
        slot = np.zeros(EVENT_RECORD, np.uint8)
        slot[:hi - lo] = a[lo:hi]
        out.append(decode(slot))
    return out
