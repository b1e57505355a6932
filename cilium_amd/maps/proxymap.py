"""pkg/maps/proxymap mirror (the reference's pkg/maps/proxymap/{proxymap,ipv4,ipv6}.go).

Proxy4Key   = struct proxy4_tbl_key   (10 B): saddr, dport, sport, nexthdr, pad
Proxy4Value = struct proxy4_tbl_value (16 B): orig_daddr, orig_dport, pad, identity, lifetime
Proxy6Key   = struct proxy6_tbl_key   (22 B), Proxy6Value = struct proxy6_tbl_value (28 B):
the same with 16-byte addresses (bpf/lib/common.h:445-475).  The port fields are u16 in
the struct's memory order; ToNetwork swaps them (the datapath stores network order).

GC (gc / gc6) deletes the entries with lifetime < tsec, Flush is gc(math.MaxUint64), and
CleanupOnRedirectClose deletes the TCP entries of a proxy port.  The reference walks the
maps with GetNextKey / LookupElement / DeleteElement; here each is one call per map,
gf_proxy_gc / gf_proxy_cleanup_port: a device sweep of the HBM replica (with probe-cluster
compaction) when the datapath owns the map, else a pass over the host shadow.  The maps
are the handles the caller holds (fd4 / fd6; None or 0: that family has no map, as when
the reference's Open fails, and counts 0).
"""
import ipaddress
import socket
import struct

from .. import bpf

Proxy4MapName, Proxy6MapName = "cilium_proxy4", "cilium_proxy6"
MaxEntries = 524288
KEY4 = struct.Struct("<4sHHBB")
VALUE4 = struct.Struct("<4sHHII")
KEY6 = struct.Struct("<16sHHBB")
VALUE6 = struct.Struct("<16sHHII")
MaxUint64 = (1 << 64) - 1


def _swap16(x):
    """byteorder.HostToNetwork(uint16) on a little-endian host."""
    return socket.htons(x & 0xFFFF)


def _ip(raw):
    """net.IP.String(): dotted quad for 4 bytes and for IPv4-mapped 16 bytes."""
    if len(raw) == 16 and raw[:12] == bytes(10) + b"\xff\xff":
        raw = raw[12:]
    return str(ipaddress.ip_address(raw))


def _join_host_port(host, port):
    """net.JoinHostPort: brackets around a host that contains a colon."""
    return f"[{host}]:{port}" if ":" in host else f"{host}:{port}"


class _Key:
    def __init__(self, SAddr=None, DPort=0, SPort=0, Nexthdr=0, Pad=0):
        self.SAddr = bytes(SAddr) if SAddr is not None else bytes(self.ALEN)
        if len(self.SAddr) != self.ALEN:
            raise ValueError(f"address of {len(self.SAddr)} bytes, expected {self.ALEN}")
        self.DPort, self.SPort, self.Nexthdr, self.Pad = DPort, SPort, Nexthdr, Pad

    def pack(self):
        return self.S.pack(self.SAddr, self.DPort, self.SPort, self.Nexthdr, self.Pad)

    @classmethod
    def unpack(cls, raw):
        return cls(*cls.S.unpack(raw))

    def ToNetwork(self):
        return type(self)(self.SAddr, _swap16(self.DPort), _swap16(self.SPort), self.Nexthdr, self.Pad)

    def HostPort(self):
        return _join_host_port(_ip(self.SAddr), self.SPort)

    def String(self):
        return f"{self.HostPort()} ({self.Nexthdr}) => {self.DPort}"

    __str__ = String

    def __eq__(self, o):
        return type(o) is type(self) and o.pack() == self.pack()

    def __hash__(self):
        return hash(self.pack())


class _Value:
    def __init__(self, OrigDAddr=None, OrigDPort=0, Pad=0, SourceIdentity=0, Lifetime=0):
        self.OrigDAddr = bytes(OrigDAddr) if OrigDAddr is not None else bytes(self.ALEN)
        if len(self.OrigDAddr) != self.ALEN:
            raise ValueError(f"address of {len(self.OrigDAddr)} bytes, expected {self.ALEN}")
        self.OrigDPort, self.Pad, self.SourceIdentity, self.Lifetime = OrigDPort, Pad, SourceIdentity, Lifetime

    def pack(self):
        return self.S.pack(self.OrigDAddr, self.OrigDPort, self.Pad, self.SourceIdentity, self.Lifetime)

    @classmethod
    def unpack(cls, raw):
        return cls(*cls.S.unpack(raw))

    def ToNetwork(self):
        return type(self)(self.OrigDAddr, _swap16(self.OrigDPort), self.Pad, self.SourceIdentity, self.Lifetime)

    def GetSourceIdentity(self):
        return self.SourceIdentity

    def HostPort(self):
        return _join_host_port(_ip(self.OrigDAddr), self.OrigDPort)

    def String(self):
        return f"{_ip(self.OrigDAddr)}:{self.OrigDPort} identity {self.SourceIdentity} lifetime {self.Lifetime}"

    __str__ = String

    def __eq__(self, o):
        return type(o) is type(self) and o.pack() == self.pack()

    def __hash__(self):
        return hash(self.pack())


class Proxy4Key(_Key):
    S, ALEN = KEY4, 4


class Proxy4Value(_Value):
    S, ALEN = VALUE4, 4


class Proxy6Key(_Key):
    S, ALEN = KEY6, 16


class Proxy6Value(_Value):
    S, ALEN = VALUE6, 16


def OpenMap(path, v6=False, max_entries=MaxEntries):
    """bpf.NewMap(Proxy{4,6}MapName, MapTypeHash, sizeof key, sizeof value, MaxEntries, 0)."""
    k, v = (KEY6, VALUE6) if v6 else (KEY4, VALUE4)
    return bpf.OpenOrCreateMap(path, bpf.BPF_MAP_TYPE_HASH, k.size, v.size, max_entries, 0)


def _family(fd4, fd6, key):
    if isinstance(key, Proxy4Key):
        return fd4, Proxy4Value
    if isinstance(key, Proxy6Key):
        return fd6, Proxy6Value
    raise TypeError(f"unknown proxymap key type: {type(key).__name__}")


def Lookup(fd4, fd6, key):
    """proxymap.Lookup -> lookupEgress{4,6}: the key in host order is looked up in network
    order, the value comes back in host order."""
    fd, vt = _family(fd4, fd6, key)
    try:
        raw = bpf.LookupElement(fd, key.ToNetwork().pack(), vt.S.size)
    except bpf.BPFError as e:
        fam = 4 if vt is Proxy4Value else 6
        raise bpf.BPFError(e.errno, f"unable to find IPv{fam} proxy entry for {key}: {e.strerror}")
    return vt.unpack(raw).ToNetwork()


def Delete(fd4, fd6, key):
    """proxymap.Delete: the key's bytes as given (the reference does not convert here)."""
    fd, _ = _family(fd4, fd6, key)
    bpf.DeleteElement(fd, key.pack())


def _gc(fd, tsec):
    if not fd:
        return 0
    from .._lib import lib
    rc = lib.gf_proxy_gc(fd, tsec, None)
    if rc < 0:
        raise bpf.BPFError(-rc, "Unable to garbage collect proxy map")
    return rc


def filter_time(time_ns):
    """gc / gc6: tsec := time / 1000000000 (uint64), compared as uint32(tsec)."""
    return ((time_ns & MaxUint64) // 1000000000) & 0xFFFFFFFF


# Flush is gc(math.MaxUint64) in the reference, so its cutoff is
# uint32(18446744073709551615 / 10^9) = uint32(18446744073) = 1266874889 and not
# 0xFFFFFFFF: an entry whose lifetime is at or past that second survives a Flush there,
# and does here.  gf_proxy_gc itself takes any u32.
FlushFilterTime = filter_time(MaxUint64)


def GC(fd4, fd6, mtime_ns):
    """proxymap.GC: gc(time) + gc6(time) with time = bpf.GetMtime() in nanoseconds; deletes
    lifetime < uint32(time / 1e9) (strict) and returns the number of entries removed."""
    t = filter_time(mtime_ns)
    return _gc(fd4, t) + _gc(fd6, t)


def Flush(fd4, fd6):
    """proxymap.Flush: gc(math.MaxUint64) + gc6(math.MaxUint64), see FlushFilterTime."""
    return _gc(fd4, FlushFilterTime) + _gc(fd6, FlushFilterTime)


def CleanupOnRedirectClose(fd4, fd6, port):
    """cleanupIPv4Redirects + cleanupIPv6Redirects: removes every entry with
    DPort == HostToNetwork(port) and Nexthdr == 6.  Returns the number removed (the
    reference returns nothing)."""
    from .._lib import lib
    n = 0
    for fd in (fd4, fd6):
        if not fd:
            continue
        rc = lib.gf_proxy_cleanup_port(fd, _swap16(port), None)
        if rc < 0:
            raise bpf.BPFError(-rc, "Unable to clean up proxy map")
        n += rc
    return n
