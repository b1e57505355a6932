"""Writes tests/golden/tunnel_kats.json (run `python tests/tunnel_kats_gen.py` to regenerate it after
adding a case below).  Every case is written out by hand as explicit field values; this script only
lays them out as lists of [field, where the field is defined, hex] and fills in the checksums, with
a sum of its own (integer arithmetic modulo 0xffff) that shares nothing with tests/tunnel_model.py
or with the fold in tests/test_tunnel_wire.py.  It knows nothing about the library."""
import json
import os
import sys

def be(v, n): return v.to_bytes(n, "big")
def csum(bs):     # one's-complement of the one's-complement sum, by integer arithmetic
    if len(bs) % 2: bs += b"\0"
    t = 0
    for i in range(0, len(bs), 2):
        t += (bs[i] << 8) | bs[i + 1]
    t = t % 0xffff if t % 0xffff or t == 0 else 0xffff      # end-around carry == mod 0xffff (0xffff for multiples)
    return 0xffff - t

CFG = {
  "vx":      dict(mode=0, flags=0, local_ip=0xC0A80A01, dst_port=8472, sport_min=32768, sport_max=61000, ttl=64, tos=0, src_mac="0200000a0001", dst_mac="020000140002"),
  "vx_ck":   dict(mode=0, flags=1, local_ip=0xC0A80A01, dst_port=8472, sport_min=32768, sport_max=61000, ttl=64, tos=0, src_mac="0200000a0001", dst_mac="020000140002"),
  "vx_df":   dict(mode=0, flags=2, local_ip=0xC0A80A01, dst_port=4789, sport_min=49152, sport_max=65535, ttl=255, tos=0xb8, src_mac="0200000a0001", dst_mac="020000140002"),
  "vx_ckdf": dict(mode=0, flags=3, local_ip=0xC0A80A01, dst_port=8472, sport_min=32768, sport_max=61000, ttl=64, tos=0, src_mac="0200000a0001", dst_mac="020000140002"),
  "vx_rx":   dict(mode=0, flags=0, local_ip=0xC0A81402, dst_port=8472, sport_min=32768, sport_max=61000, ttl=64, tos=0, src_mac="020000140002", dst_mac="0200000a0001"),
  "gn":      dict(mode=1, flags=0, local_ip=0x0A000001, dst_port=6081, sport_min=32768, sport_max=61000, ttl=64, tos=0, src_mac="0200000a0001", dst_mac="020000140002"),
  "gn_ck":   dict(mode=1, flags=1, local_ip=0x0A000001, dst_port=6081, sport_min=32768, sport_max=61000, ttl=64, tos=0, src_mac="0200000a0001", dst_mac="020000140002"),
  "gn_ckdf": dict(mode=1, flags=3, local_ip=0x0A000001, dst_port=6081, sport_min=1024, sport_max=1024, ttl=1, tos=4, src_mac="0200000a0001", dst_mac="020000140002"),
  "gn_any":  dict(mode=1, flags=0, local_ip=0, dst_port=6081, sport_min=32768, sport_max=61000, ttl=64, tos=0, src_mac="0200000a0001", dst_mac="020000140002"),
}

def inner(L, S):
    b = bytearray((i * 7 + 3) & 0xff for i in range(max(L, S)))
    if len(b) >= 14: b[12], b[13] = 0x08, 0x00
    snap = bytes(b[:S]).ljust(S, b"\0")
    return snap

def outer(c, inner_bytes, L, remote, tid, opt=b"", fh=0, ipid=0, dmac=None, ihl=5, ipopt=b"", fix=None):
    """fields of the outer frame; fix(dict) may override raw field values before checksums."""
    c = CFG[c]
    geneve = c["mode"] == 1
    ol = len(opt)
    tunlen = 8 + ol
    ulen = 8 + tunlen + L
    tot = 4 * ihl + ulen
    sport = c["sport_min"] + ((fh * (c["sport_max"] - c["sport_min"])) >> 32)
    v = dict(dmac=bytes.fromhex(dmac or c["dst_mac"]), smac=bytes.fromhex(c["src_mac"]), etype=b"\x08\x00",
             vihl=bytes([0x40 | ihl]), tos=bytes([c["tos"]]), tot=be(tot, 2), id=be(ipid, 2),
             frag=be(0x4000 if c["flags"] & 2 else 0, 2), ttl=bytes([c["ttl"]]), proto=b"\x11", saddr=be(c["local_ip"] or 0x0A000063, 4),
             daddr=be(remote, 4), ipopt=ipopt, sport=be(sport, 2), dport=be(c["dst_port"], 2), ulen=be(ulen, 2))
    if geneve:
        v.update(t0=bytes([ol // 4]), t1=b"\0", tproto=b"\x65\x58", vni=be(tid & 0xffffff, 3), trsvd=b"\0", opts=opt)
    else:
        v.update(t0=b"\x08", t1=b"\0\0\0", vni=be(tid & 0xffffff, 3), trsvd=b"\0")
    if fix: v.update({k: x for k, x in fix.items() if k in v})
    iph = v["vihl"] + v["tos"] + v["tot"] + v["id"] + v["frag"] + v["ttl"] + v["proto"] + b"\0\0" + v["saddr"] + v["daddr"] + v["ipopt"]
    v["ipck"] = be(csum(iph), 2)
    tun = v["t0"] + v["t1"] + (v["tproto"] if geneve else b"") + v["vni"] + v["trsvd"] + (v["opts"] if geneve else b"")
    v["uck"] = b"\0\0"
    if c["flags"] & 1 or (fix and fix.get("force_ck")):
        ps = v["saddr"] + v["daddr"] + b"\0\x11" + v["ulen"]
        ck = csum(ps + v["sport"] + v["dport"] + v["ulen"] + b"\0\0" + tun + inner_bytes[:L])
        v["uck"] = be(ck or 0xffff, 2)
    if fix:
        for k in ("ipck", "uck"):
            if k in fix: v[k] = fix[k]
    F = [["outer destination MAC", "IEEE 802.3", v["dmac"]], ["outer source MAC", "IEEE 802.3", v["smac"]],
         ["EtherType IPv4", "RFC 894", v["etype"]],
         ["Version 4, IHL %d" % ihl, "RFC 791 3.1", v["vihl"]], ["Type of Service", "RFC 791 3.1", v["tos"]],
         ["Total Length", "RFC 791 3.1", v["tot"]], ["Identification", "RFC 791 3.1", v["id"]],
         ["Flags (DF 0x4000) and Fragment Offset", "RFC 791 3.1", v["frag"]], ["Time to Live", "RFC 791 3.1", v["ttl"]],
         ["Protocol 17 (UDP)", "RFC 791 3.1", v["proto"]], ["Header Checksum", "RFC 791 3.1", v["ipck"]],
         ["Source Address", "RFC 791 3.1", v["saddr"]], ["Destination Address", "RFC 791 3.1", v["daddr"]]]
    if v["ipopt"]: F.append(["Options (No Operation x4)", "RFC 791 3.1", v["ipopt"]])
    F += [["Source Port", "RFC 768", v["sport"]], ["Destination Port", "RFC 768", v["dport"]], ["Length", "RFC 768", v["ulen"]],
          ["Checksum (0 = none; computed 0 sent as ffff)", "RFC 768", v["uck"]]]
    if geneve:
        F += [["Ver 0, Opt Len (4-byte words)", "RFC 8926 3.4", v["t0"]], ["O, C, Rsvd", "RFC 8926 3.4", v["t1"]],
              ["Protocol Type 0x6558", "RFC 8926 3.4", v["tproto"]], ["VNI", "RFC 8926 3.4", v["vni"]],
              ["Reserved", "RFC 8926 3.4", v["trsvd"]]]
        if v["opts"]: F.append(["Variable-Length Options", "RFC 8926 3.5", v["opts"]])
    else:
        F += [["Flags (I = 0x08)", "RFC 7348 5", v["t0"]], ["Reserved", "RFC 7348 5", v["t1"]], ["VNI", "RFC 7348 5", v["vni"]],
              ["Reserved", "RFC 7348 5", v["trsvd"]]]
    return F

def hexf(F): return [[a, b, c.hex()] for a, b, c in F]
def cat(F): return b"".join(c for _, _, c in F)

S, OS = 64, 128
OPT8 = bytes.fromhex("ffff01010000011e")
OPT64 = bytes((0x40 + i) & 0xff for i in range(64))
enc, dec = [], []

def E(name, cfg, L, remote=0xC0A81402, tid=0x0000011e, opt=b"", opt_len=None, opt_stride=0, select=1, fh=0, ipid=0, dmac=None,
      status=0, snap=None, S=S, OS=OS):
    snap = snap if snap is not None else inner(L, S)
    ol = len(opt) if opt_len is None else opt_len
    row = None
    if status == 0:
        F = outer(cfg, snap, L, remote, tid, opt[:ol], fh, ipid, dmac)
        payload = snap[:min(L, S)]
        F.append(["inner frame (first min(len, snap_stride) bytes)", "RFC 7348 5 / RFC 8926 3", payload])
        row = F
    enc.append(dict(name=name, cfg=cfg, snap_stride=S, out_stride=OS, frame=snap.hex(), len=L, remote_ip=remote, tunnel_id=tid,
                    opt=opt.ljust(opt_stride, b"\0").hex() if opt_stride else "", opt_len=ol, opt_stride=opt_stride, select=select,
                    flow_hash=fh, ip_id=ipid, dst_mac=dmac, status=status, out_len=(L + 50 + ol) if status == 0 else 0,
                    outer=hexf(row) if row else None))
    return row

E("vxlan len 14", "vx", 14)
E("vxlan len 14, checksum and DF", "vx_ckdf", 14)
E("vxlan len 15 (odd: the checksum's tail byte)", "vx_ck", 15)
E("vxlan len 15, DF, port 4789, TOS and TTL set", "vx_df", 15)
E("vxlan len == snap_stride, checksum", "vx_ck", 64)
E("vxlan len > snap_stride without checksum: lengths from len, bytes from the snap", "vx", 100)
E("vxlan len > snap_stride with checksum", "vx_ck", 100, status=4)
E("geneve no options, checksum", "gn_ck", 40, tid=0xABCDEF12)
E("geneve opt_len 8, checksum and DF, one-port range, TTL 1", "gn_ckdf", 33, opt=OPT8, opt_stride=8, fh=0xdeadbeef)
E("geneve opt_len 8, no checksum", "gn", 20, opt=OPT8, opt_stride=8)
E("geneve opt_len 64, len 14: the headers fill out_stride", "gn_ck", 14, opt=OPT64, opt_stride=64)
E("geneve opt_len 64, len 64: the row is cut at out_stride", "gn", 64, opt=OPT64, opt_stride=64)
E("geneve opt_len 6", "gn", 20, opt=OPT8, opt_len=6, opt_stride=8, status=3)
E("geneve opt_len 12 > opt_stride 8", "gn", 20, opt=OPT8, opt_len=12, opt_stride=8, status=3)
E("geneve opt_len 68 > 64", "gn", 20, opt=OPT64, opt_len=68, opt_stride=64, status=3)
E("not selected", "vx_ck", 40, select=0, status=1)
E("len 13", "vx", 13, status=2)
E("vxlan flow_hash, ip_id and dst_mac columns", "vx_ck", 41, fh=0x80000000, ipid=0xbeef, dmac="0a0b0c0d0e0f")
E("geneve flow_hash ffffffff: the last port below sport_max", "gn", 30, fh=0xffffffff, tid=0xffffffff)
# a computed UDP checksum of 0: choose the inner frame's last two bytes so that the sum is 0xffff
L = 32
sn = bytearray(inner(L, S))
sn[30] = sn[31] = 0
F = outer("vx_ck", bytes(sn), L, 0xC0A81402, 0x11e)
ck = int.from_bytes(dict((a, c) for a, _, c in F)["Checksum (0 = none; computed 0 sent as ffff)"], "big")
# ck = ~sum; adding word w makes the sum's complement 0 when w == ck (sum + ck == 0xffff)
sn[30], sn[31] = ck >> 8, ck & 0xff
r0 = E("vxlan computed checksum 0 is sent as ffff", "vx_ck", L, snap=bytes(sn))
assert dict((a, c) for a, _, c in r0)["Checksum (0 = none; computed 0 sent as ffff)"] == b"\xff\xff", r0

def D(name, cfg, F, L=None, status=0, S=128, IS=64, opt_stride=8, inner_len=None, inner_b=None, tid=None, saddr=None, ol=None, opt=None, raw=None):
    fr = cat(F) if raw is None else raw
    L = len(fr) if L is None else L
    want = dict(status=status, inner_len=inner_len if inner_len is not None else 0)
    if status in (0, 9):
        want.update(inner=inner_b.hex(), tunnel_id=tid, outer_saddr=saddr, opt_len=ol, opt=(opt or b"").hex())
    dec.append(dict(name=name, cfg=cfg, snap_stride=S, inner_stride=IS, opt_stride=opt_stride, len=L, outer=hexf(F), want=want))

def O(cfg, L, remote, tid=0x11e, opt=b"", **kw):
    snap = inner(L, max(L, 1))
    F = outer(cfg, snap, L, remote, tid, opt, **kw)
    F.append(["inner frame", "RFC 7348 5 / RFC 8926 3", snap[:L]])
    return F, snap[:L]

ME_VX, ME_GN = 0xC0A80A01, 0x0A000001      # the receivers' local_ip (== the senders': both ends share the KAT config)
F, i = O("vx", 30, ME_VX)
D("vxlan, no checksum", "vx", F, inner_len=30, inner_b=i, tid=0x11e, saddr=ME_VX, ol=0)
F, i = O("vx_ck", 31, ME_VX, tid=0xfedcba)
D("vxlan, checksum verified (odd length)", "vx", F, inner_len=31, inner_b=i, tid=0xfedcba, saddr=ME_VX, ol=0)
F, i = O("gn_ck", 40, ME_GN, opt=OPT8)
D("geneve opt_len 8, checksum verified", "gn", F, inner_len=40, inner_b=i, tid=0x11e, saddr=ME_GN, ol=8, opt=OPT8)
F, i = O("gn", 20, ME_GN, opt=OPT64[:16])
D("geneve opt_len 16 > opt_stride 8: the first 8 option bytes", "gn", F, inner_len=20, inner_b=i, tid=0x11e, saddr=ME_GN, ol=16, opt=OPT64[:8])
F, i = O("gn", 20, 0x0A0000FE)
D("geneve, local_ip 0 accepts any daddr", "gn_any", F, inner_len=20, inner_b=i, tid=0x11e, saddr=ME_GN, ol=0)
F, i = O("vx", 30, ME_VX, fix=dict(etype=b"\x86\xdd"))
D("ethertype 86dd", "vx", F, status=5)
F, i = O("vx", 30, ME_VX, fix=dict(proto=b"\x06"))
D("protocol 6", "vx", F, status=5)
F, i = O("vx", 30, ME_VX, fix=dict(frag=b"\x20\x00"))
D("a fragment: MF set", "vx", F, status=5)
F, i = O("vx", 30, ME_VX, fix=dict(frag=b"\x00\x10"))
D("a fragment: offset 16", "vx", F, status=5)
F, i = O("vx", 30, 0xC0A80A02)
D("daddr is not local_ip", "vx", F, status=5)
F, i = O("vx_df", 30, ME_VX)
D("destination port 4789 at an 8472 endpoint", "vx", F, status=5)
F, i = O("vx", 30, ME_VX, fix=dict(ipck=b"\x12\x34"))
D("IPv4 header checksum wrong", "vx", F, status=6)
F, i = O("vx", 30, ME_VX, fix=dict(tot=be(20 + 8 + 8 + 30 + 1, 2)))
D("IPv4 total length disagrees with len", "vx", F, status=6)
F, i = O("vx", 30, ME_VX, fix=dict(ulen=be(8 + 8 + 30 - 2, 2)))
D("UDP length disagrees with len", "vx", F, status=6)
F, i = O("vx", 30, ME_VX, fix=dict(vihl=b"\x65"))
D("version 6", "vx", F, status=6)
F, i = O("vx", 30, ME_VX, fix=dict(vihl=b"\x44"))
D("IHL 4", "vx", F, status=6)
F, i = O("vx", 30, ME_VX)
D("frame shorter than its headers (len 45)", "vx", F, L=45, status=6, raw=cat(F)[:45])
dec[-1]["outer"] = hexf(F)
dec[-1]["cut"] = 45
F, i = O("vx_ck", 30, ME_VX, ihl=6, ipopt=b"\x01\x01\x01\x01")
D("outer IHL 6 is accepted and skipped, checksum verified", "vx", F, inner_len=30, inner_b=i, tid=0x11e, saddr=ME_VX, ol=0)
F, i = O("vx", 30, ME_VX, fix=dict(t0=b"\x00"))
D("vxlan I bit clear", "vx", F, status=7)
F, i = O("vx", 30, ME_VX, fix=dict(t1=b"\x00\x00\x01"))
D("vxlan reserved bit set", "vx", F, status=7)
F, i = O("vx", 30, ME_VX, fix=dict(trsvd=b"\x80"))
D("vxlan reserved byte after the VNI set", "vx", F, status=7)
F, i = O("gn", 30, ME_GN, fix=dict(t0=b"\x40"))
D("geneve version 1", "gn", F, status=7)
F, i = O("gn", 30, ME_GN, fix=dict(t1=b"\x40"))
D("geneve C bit (critical options)", "gn", F, status=7)
F, i = O("gn", 30, ME_GN, fix=dict(t1=b"\x80"))
D("geneve O bit is ignored", "gn", F, inner_len=30, inner_b=i, tid=0x11e, saddr=ME_GN, ol=0)
F, i = O("gn", 30, ME_GN, fix=dict(tproto=b"\x08\x00"))
D("geneve protocol 0x0800", "gn", F, status=7)
F, i = O("gn", 8, ME_GN, fix=dict(t0=b"\x03"))
D("geneve options (12 B) run past the datagram (8 B left)", "gn", F, status=7)
F, i = O("vx_ck", 30, ME_VX)
F[-1][2] = bytes([F[-1][2][0] ^ 1]) + F[-1][2][1:]
D("UDP checksum wrong (one inner bit flipped)", "vx", F, status=8)
F, i = O("vx_ck", 200, ME_VX)
D("checksum present, datagram longer than the snap", "vx", F, status=9, S=128, inner_len=200, inner_b=i[:64], tid=0x11e, saddr=ME_VX, ol=0)
F, i = O("vx", 200, ME_VX)
D("no checksum, datagram longer than the snap: the inner bytes inside it", "vx", F, S=64, IS=64, inner_len=200, inner_b=i[:14], tid=0x11e, saddr=ME_VX, ol=0)
F = [[a, b, c] for a, b, c in r0]
D("a checksum sent as ffff verifies (at the peer, 192.168.20.2)", "vx_rx", F, inner_len=32, inner_b=bytes(sn[:32]), tid=0x11e, saddr=ME_VX, ol=0)

doc = {"comment": "Known answers of gf_tunnel_encap / gf_tunnel_decap, written by tests/tunnel_kats_gen.py from the cases listed "
       "there.  Each outer frame is a list of [field, where the field is "
       "defined, bytes as hex] in wire order; the frame is their concatenation.  Built field by field from the RFCs cited, "
       "every checksum recomputed in full.  encap: 'outer' = the bytes written at the start of the output row (cut at "
       "out_stride by the test), null = the row is not written.  decap: 'cut' = only that many bytes of the listed frame are "
       "on the wire.  Addresses and ids are numbers (192.168.10.1 = 3232238081).  Statuses: GF_TUN_ST_* of include/gpuflow.h.",
       "cfgs": CFG, "encap": enc, "decap": dec}
path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tunnel_kats.json")
json.dump(doc, open(path, "w"), indent=1)
print(len(enc), len(dec))
