"""VXLAN / Geneve encapsulation and decapsulation per frame, restated from the RFCs in plain
Python: the checker of gf_tunnel_encap / gf_tunnel_decap (include/gpuflow.h has the rules).

  RFC 791  section 3.1   the IPv4 header and its checksum
  RFC 768                the UDP header, the pseudo-header, checksum 0 = none, computed 0 sent as 0xffff
  RFC 7348 section 5     the VXLAN header: flags 0x08 (I), 24 reserved bits, VNI, 8 reserved bits
  RFC 8926 section 3.4   the Geneve header: Ver(2) OptLen(6) | O C Rsvd(6) | protocol 0x6558 | VNI | Rsvd(8)

Nothing here knows the device code: frames are bytes, fields are written with struct.pack in
network order, and sums are taken over the finished byte strings.
"""
import struct
from types import SimpleNamespace

import numpy as np

VXLAN, GENEVE = 0, 1
F_UDP_CSUM, F_DF = 1, 2
(ST_OK, ST_SKIPPED, ST_SHORT, ST_BAD_OPT, ST_TRUNCATED, ST_NOT_TUNNEL, ST_BAD_OUTER, ST_BAD_HDR, ST_BAD_CSUM,
 ST_OK_UNVERIFIED) = range(10)
POISON = 0xA5


def cfg(mode, dst_port, local_ip=0, flags=0, sport_min=32768, sport_max=61000, ttl=64, tos=0,
        src_mac=bytes(6), dst_mac=bytes(6)):
    return SimpleNamespace(mode=mode, dst_port=dst_port, local_ip=local_ip, flags=flags, sport_min=sport_min,
                           sport_max=sport_max, ttl=ttl, tos=tos, src_mac=bytes(src_mac), dst_mac=bytes(dst_mac))


def ones_sum(data):
    """RFC 1071: the one's-complement sum of the 16-bit big-endian words, an odd byte padded with 0."""
    if len(data) & 1:
        data = data + b"\0"
    s = sum(struct.unpack("!%dH" % (len(data) // 2), data))
    while s >> 16:
        s = (s & 0xffff) + (s >> 16)
    return s


def encap(c, snap, length, remote_ip, tunnel_id, out_stride, opt=b"", opt_len=0, opt_stride=0, select=1, flow_hash=0,
          ip_id=0, dst_mac=None):
    """One frame.  snap: its snap_stride bytes; opt: its row of the option column (Geneve, b"" = no
    column).  Returns (status, out_len, row): row = the bytes the call writes at the start of the
    output row (None unless OK)."""
    S = len(snap)
    ol = 0
    if not select:
        return ST_SKIPPED, 0, None
    if length < 14:
        return ST_SHORT, 0, None
    if c.mode == GENEVE and opt_stride:
        ol = opt_len
        if ol % 4 or ol > opt_stride or ol > 64:
            return ST_BAD_OPT, 0, None
    if c.flags & F_UDP_CSUM and length > S:
        return ST_TRUNCATED, 0, None
    inner = bytes(snap[:min(length, S)])
    vni = tunnel_id & 0xffffff
    if c.mode == GENEVE:
        tun = struct.pack("!BBHI", ol // 4, 0, 0x6558, vni << 8) + bytes(opt[:ol])
    else:
        tun = struct.pack("!II", 0x08 << 24, vni << 8)
    ulen = (8 + len(tun) + length) & 0xffff
    tot = (20 + 8 + len(tun) + length) & 0xffff
    sport = c.sport_min + ((flow_hash * (c.sport_max - c.sport_min)) >> 32)
    ip = struct.pack("!BBHHHBBHII", 0x45, c.tos, tot, ip_id, 0x4000 if c.flags & F_DF else 0, c.ttl, 17, 0,
                     c.local_ip, remote_ip)
    ip = ip[:10] + struct.pack("!H", ~ones_sum(ip) & 0xffff) + ip[12:]
    udp = struct.pack("!HHHH", sport, c.dst_port, ulen, 0)
    if c.flags & F_UDP_CSUM:
        pseudo = ip[12:20] + struct.pack("!BBH", 0, 17, ulen)
        ck = ~ones_sum(pseudo + udp + tun + inner) & 0xffff
        udp = udp[:6] + struct.pack("!H", ck or 0xffff)
    eth = (bytes(dst_mac) if dst_mac is not None else c.dst_mac) + c.src_mac + b"\x08\x00"
    full = eth + ip + udp + tun + inner
    return ST_OK, length + 50 + ol, full[:out_stride]


def decap(c, snap, length, inner_stride, opt_stride=0):
    """One outer frame.  Returns a namespace: status, inner_len, and for OK / OK_UNVERIFIED inner (the
    bytes written at the start of the row), tunnel_id, outer_saddr, opt_len, opt (the bytes written
    at the start of the option row)."""
    S = len(snap)
    cap = min(length, S)
    f = bytes(snap[:cap])
    r = SimpleNamespace(status=ST_OK, inner_len=0, inner=None, tunnel_id=None, outer_saddr=None, opt_len=None, opt=None)

    def end(st):
        r.status = st
        return r
    if cap < 14:
        return end(ST_BAD_OUTER)
    if f[12:14] != b"\x08\x00":
        return end(ST_NOT_TUNNEL)
    if cap < 34:
        return end(ST_BAD_OUTER)
    vi, _, tot, _, fo, _, proto, _, saddr, daddr = struct.unpack("!BBHHHBBHII", f[14:34])
    if proto != 17 or fo & 0x3fff or (c.local_ip and daddr != c.local_ip):
        return end(ST_NOT_TUNNEL)
    ihl = vi & 15
    if vi >> 4 != 4 or ihl < 5:
        return end(ST_BAD_OUTER)
    l4 = 14 + 4 * ihl
    if l4 + 8 > cap:
        return end(ST_BAD_OUTER)
    _, dport, ulen, ck = struct.unpack("!HHHH", f[l4:l4 + 8])
    if dport != c.dst_port:
        return end(ST_NOT_TUNNEL)
    if tot != length - 14 or ulen != length - l4 or l4 + 16 > cap:
        return end(ST_BAD_OUTER)
    if ones_sum(f[14:l4]) != 0xffff:
        return end(ST_BAD_OUTER)
    t = f[l4 + 8:l4 + 16]
    ol = 0
    if c.mode == VXLAN:
        if t[0] != 0x08 or t[1:4] != b"\0\0\0" or t[7]:
            return end(ST_BAD_HDR)
    else:
        ol = (t[0] & 0x3f) * 4
        if t[0] >> 6 or t[1] & 0x40 or t[2:4] != b"\x65\x58" or l4 + 16 + ol > cap:
            return end(ST_BAD_HDR)
    off = l4 + 16 + ol
    if ck:
        if length <= S:
            pseudo = f[26:34] + struct.pack("!BBH", 0, 17, ulen)
            if ones_sum(pseudo + f[l4:length]) != 0xffff:
                return end(ST_BAD_CSUM)
        else:
            r.status = ST_OK_UNVERIFIED
    r.inner_len = length - off
    r.inner = f[off:][:inner_stride]
    r.tunnel_id = int.from_bytes(t[4:7], "big")
    r.outer_saddr = saddr
    r.opt_len = ol
    r.opt = f[l4 + 16:l4 + 16 + min(ol, opt_stride)] if c.mode == GENEVE else b""
    return r


# ---------------------------------------------------------------- batches (numpy in, numpy out)
def encap_batch(c, frames, lens, remote_ip, tunnel_id, out_stride, opt=None, opt_len=None, select=None, flow_hash=None,
                ip_id=None, dst_mac=None, poison=POISON):
    """The call over a batch: (out [n,out_stride] u8 starting as poison, out_len [n] u32, status [n] u8)."""
    n = len(lens)
    out = np.full((n, out_stride), poison, np.uint8)
    out_len, status = np.zeros(n, np.uint32), np.zeros(n, np.uint8)
    for i in range(n):
        st, ln, row = encap(c, frames[i].tobytes(), int(lens[i]), int(remote_ip[i]), int(tunnel_id[i]), out_stride,
                            opt[i].tobytes() if opt is not None else b"", int(opt_len[i]) if opt is not None else 0,
                            opt.shape[1] if opt is not None else 0, 1 if select is None else int(select[i]),
                            0 if flow_hash is None else int(flow_hash[i]), 0 if ip_id is None else int(ip_id[i]),
                            None if dst_mac is None else dst_mac[i].tobytes())
        status[i], out_len[i] = st, ln
        if row is not None:
            out[i, :len(row)] = np.frombuffer(row, np.uint8)
    return out, out_len, status


def decap_batch(c, frames, lens, inner_stride, opt_stride=8, poison=POISON):
    """The call over a batch, every output starting as poison: a namespace of inner [n,inner_stride],
    inner_len, tunnel_id, outer_saddr (u32), opt [n,opt_stride], opt_len, status (u8)."""
    n = len(lens)
    p32 = poison * 0x01010101
    r = SimpleNamespace(inner=np.full((n, inner_stride), poison, np.uint8), inner_len=np.zeros(n, np.uint32),
                        tunnel_id=np.full(n, p32, np.uint32), outer_saddr=np.full(n, p32, np.uint32),
                        opt=np.full((n, opt_stride), poison, np.uint8), opt_len=np.full(n, poison, np.uint8),
                        status=np.zeros(n, np.uint8))
    for i in range(n):
        d = decap(c, frames[i].tobytes(), int(lens[i]), inner_stride, opt_stride)
        r.status[i], r.inner_len[i] = d.status, d.inner_len
        if d.inner is not None:
            r.inner[i, :len(d.inner)] = np.frombuffer(d.inner, np.uint8)
            r.tunnel_id[i], r.outer_saddr[i], r.opt_len[i] = d.tunnel_id, d.outer_saddr, d.opt_len
            r.opt[i, :len(d.opt)] = np.frombuffer(d.opt, np.uint8)
    return r
