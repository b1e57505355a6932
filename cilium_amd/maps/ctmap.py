"""pkg/maps/ctmap mirror (/root/reference/pkg/maps/ctmap/{ctmap,ipv4,ipv6}.go).

CtKey4Global = struct ipv4_ct_tuple (14 B, packed): daddr, saddr, dport(be), sport(be), nexthdr, flags
CtKey6Global = struct ipv6_ct_tuple (40 B)
CtEntry (48 B): rx_packets, rx_bytes, tx_packets, tx_bytes, lifetime u32, flags u16,
                revnat u16 (network order), unused u16, pad u16, src_sec_id u32
GC (ctmap.go:277-352) deletes entries whose lifetime < now; Flush (:354-368)
deletes every entry.  Both go to gf_ct_gc: a device sweep of the HBM replica
(with probe-cluster compaction) when the datapath owns the map.  GCMaps / GCRound
collect many maps in one gf_ct_gc_maps call: one iteration of the agent's loop over
every endpoint's local pair and the global pair (pkg/endpointmanager/conntrack.go:84-130).
"""
import errno
import struct

from .. import bpf

MapName6, MapName4 = "cilium_ct6_", "cilium_ct4_"
MapName6Global, MapName4Global = MapName6 + "global", MapName4 + "global"
MapNumEntriesLocal, MapNumEntriesGlobal = 64000, 1000000
TUPLE_F_OUT, TUPLE_F_IN, TUPLE_F_RELATED = 0, 1, 2
KEY4 = struct.Struct("<IIHHBB")
KEY6 = struct.Struct("<16s16sHHBB2s")
ENTRY = struct.Struct("<QQQQIHHHHI")


def MapNames(ep_id=None, local=False):
    """The CT maps an endpoint's program binds (pkg/endpoint/bpf.go:268-276): with the
    ConntrackLocal option its own cilium_ct6_<id> / cilium_ct4_<id> of CT_MAP_SIZE
    MapNumEntriesLocal, else the global ones of MapNumEntriesGlobal.  Returns
    (CT_MAP6 name, CT_MAP4 name, CT_MAP_SIZE); the classify calls take either kind, mixed
    in one program array (include/gpuflow.h, gf_lxc_cfg.ct_map4)."""
    if local:
        if ep_id is None:
            raise ValueError("a per-endpoint CT map needs the endpoint ID")
        return MapName6 + str(int(ep_id)), MapName4 + str(int(ep_id)), MapNumEntriesLocal
    return MapName6Global, MapName4Global, MapNumEntriesGlobal


def ct_key4(daddr_be, saddr_be, dport_be, sport_be, nexthdr, flags):
    return KEY4.pack(daddr_be, saddr_be, dport_be, sport_be, nexthdr, flags)


def ct_key6(daddr, saddr, dport_be, sport_be, nexthdr, flags):
    return KEY6.pack(daddr, saddr, dport_be, sport_be, nexthdr, flags, b"\x00\x00")


def ct_entry(rx_packets=0, rx_bytes=0, tx_packets=0, tx_bytes=0, lifetime=0, flags=0,
             revnat=0, src_sec_id=0):
    return ENTRY.pack(rx_packets, rx_bytes, tx_packets, tx_bytes, lifetime, flags, revnat, 0, 0, src_sec_id)


class CtEntry:
    def __init__(self, raw):
        (self.rx_packets, self.rx_bytes, self.tx_packets, self.tx_bytes, self.lifetime, self.flags,
         self.revnat, self.unused, _, self.src_sec_id) = ENTRY.unpack(raw)


def OpenMap(path, v6=False, max_entries=MapNumEntriesGlobal, lru=True):
    typ = bpf.BPF_MAP_TYPE_LRU_HASH if lru else bpf.BPF_MAP_TYPE_HASH
    ks = KEY6.size if v6 else KEY4.size
    fd, new = bpf.OpenOrCreateMap(path, typ, ks, ENTRY.size, max_entries, 0)
    return fd, new


def Dump(fd, v6=False):
    ks = KEY6.size if v6 else KEY4.size
    out = []
    key = None
    while True:
        try:
            nk = bpf.GetNextKey(fd, key, ks)
        except bpf.BPFError as e:
            if e.errno == errno.ENOENT:
                return out
            raise
        out.append((nk, CtEntry(bpf.LookupElement(fd, nk, ENTRY.size))))
        key = nk


MaxTime = 0xFFFFFFFF


def GC(fd, now_sec, v6=False):
    """doGC4/doGC6 + doFiltering (GCFilterByTime): delete lifetime < now; returns
    the number of entries deleted."""
    from .._lib import lib
    rc = lib.gf_ct_gc(fd, now_sec & 0xFFFFFFFF, None)
    if rc < 0:
        raise bpf.BPFError(-rc, "Unable to garbage collect CT map")
    return rc


def Flush(fd, v6=False):
    """ctmap.Flush: GC with filter time MaxTime (every entry)."""
    return GC(fd, MaxTime, v6)


def EvictLog(fd, max_records=4096):
    """gf_ct_evict_log: the LRU stand-in's evictions of a CT map, oldest first, as
    (seq, now_sec, age_cut, hand_line, lines, evicted) tuples (include/gpuflow.h,
    gf_ct_evict_rec); at most max_records of them."""
    from .._lib import lib, gf_ct_evict_rec
    recs = (gf_ct_evict_rec * max_records)()
    n = lib.gf_ct_evict_log(fd, recs, max_records)
    if n < 0:
        raise bpf.BPFError(-n, "Unable to read the CT map's eviction log")
    return [(r.seq, r.now_sec, r.age_cut, r.hand_line, r.lines, r.evicted) for r in recs[:min(n, max_records)]]


def GCMaps(fds, now_sec, stream=None):
    """GC over many CT maps in one gf_ct_gc_maps call (IPv4 and IPv6, LRU and HASH,
    host- and device-owned maps mixed; each map at most once).  Returns the number of
    entries deleted from each map, in the order of `fds`."""
    import ctypes as C
    from .._lib import lib
    fds = [int(f) for f in fds]
    n = len(fds)
    arr = (C.c_int * max(n, 1))(*fds)
    out = (C.c_uint32 * max(n, 1))()
    rc = lib.gf_ct_gc_maps(arr, n, now_sec & 0xFFFFFFFF, out, stream)
    if rc < 0:
        raise bpf.BPFError(-rc, "Unable to garbage collect CT maps")
    return list(out[:n])


def GCRound(endpoints, now_sec, ipv4=True, ipv6=True, open_map=None):
    """One iteration of the agent's GC loop (EnableConntrackGC,
    pkg/endpointmanager/conntrack.go:84-130) over `endpoints`, an iterable of
    (ep_id, conntrack_local): an endpoint with ConntrackLocal contributes its own
    cilium_ct6_<id> / cilium_ct4_<id> (MapNames), and the global pair is collected
    once per round however many endpoints share it (seenGlobal).  Every map goes
    through one GCMaps call.  open_map(name, v6, max_entries) returns the map's
    handle, which stays the caller's, or None to leave that map out; the default is
    RunGC's (:64-70): the pinned map is opened, a map that is not there is left out,
    and the handles are closed after the round.  Returns {map name: deleted}."""
    own = open_map is None

    def pinned(name, v6, max_entries):
        try:
            return bpf.ObjGet(bpf.MapPath(name))
        except bpf.BPFError:
            return None

    names, fds, seen_global = [], [], False
    try:
        for ep_id, local in endpoints:
            if not local:
                if seen_global:
                    continue
                seen_global = True
            name6, name4, size = MapNames(ep_id, local=local)
            for on, name, v6 in ((ipv6, name6, True), (ipv4, name4, False)):
                fd = (pinned if own else open_map)(name, v6, size) if on else None
                if fd is not None:
                    names.append(name)
                    fds.append(fd)
        return dict(zip(names, GCMaps(fds, now_sec)))
    finally:
        if own:
            for fd in fds:
                bpf.ObjClose(fd)
