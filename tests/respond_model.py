"""Per-frame restatement of the ARP / ICMPv6 responder tail calls, written from the reference
text (bpf/lib/arp.h:34-95, bpf/lib/icmp6.h:43-361, bpf/lib/ipv6.h:262-274, bpf/lib/drop.h:117-120;
bpf_skb_change_tail, bpf_l4_csum_replace and bpf_csum_diff of Linux net/core/filter.c), the checker
of gf_respond where the CPU oracle has nothing to say, and a generator of well-formed and malformed
responder frames.

The skb is a bytearray that grows and shrinks (skb_change_tail) and fails loads / stores past its
length; only afterwards is it cut or zero-padded to the snap stride.  Checksums are kept in network
order, as 16-bit one's-complement arithmetic: bpf_l4_csum_replace(off, 0, diff, BPF_F_PSEUDO_HDR) is
csum_fold(csum_add(diff, ~csum_unfold(old))), whose 32-bit operand is never 0 (the upper half of
~csum_unfold is 0xffff), so the folded sum is the residue mod 0xffff with 0 represented as 0xffff.
"""
import struct

import numpy as np

RESP_OUT = np.dtype([("action", "u1"), ("reason", "u1"), ("call", "u1"), ("pad", "u1"), ("len", "<u4")])
TC_OK, TC_SHOT, TC_REDIRECT = 0, 2, 7
CALL_NONE, CALL_ARP, CALL_NS, CALL_ECHO, CALL_TE = range(5)
DROP_INVALID, DROP_MISSED_TAIL_CALL, DROP_WRITE_ERROR, DROP_UNKNOWN_L4 = 134, 140, 141, 142
DROP_UNKNOWN_TARGET, DROP_CSUM_L4 = 150, 154
F_NS_TO_STACK = 1
PAYLOAD = 128            # TRACE_PAYLOAD_LEN
EVENT_RECORD = 160


class Cfg:
    """The constants the calls read: IPV4_GATEWAY (4 bytes, network order), ROUTER_IP (16),
    the node's NODE_MAC (6), and per cilium_policy slot (NODE_MAC, LXC_ID) of its program."""

    def __init__(self, gateway, router, node_mac, progs=None, flags=0, max_len=0):
        self.gateway, self.router, self.node_mac = bytes(gateway), bytes(router), bytes(node_mac)
        self.progs = dict(progs or {})
        self.flags, self.max_len = flags, max_len or 1514


class Drop(Exception):
    def __init__(self, reason):
        self.reason = reason


class Skb:
    def __init__(self, data, length, stride):
        # bytes past the snap are not captured: they read as 0 and swallow writes
        self.stride = stride
        self.len = length
        self.b = bytearray(data[:stride])

    def load(self, off, n, err=DROP_INVALID):
        if off + n > self.len:
            raise Drop(err)
        return bytes(self.b[off:off + n]).ljust(n, b"\0")

    def store(self, off, data, err=DROP_WRITE_ERROR):
        if off + len(data) > self.len:
            raise Drop(err)
        for k, v in enumerate(data):
            if off + k < self.stride:
                self.b[off + k] = v

    def change_tail(self, new_len, max_len):
        new_len &= 0xFFFFFFFF                  # u32 new_len = skb->len + trimlen
        if new_len > max_len or new_len < 54:  # __bpf_skb_max_len / __bpf_skb_min_len (network offset + ipv6hdr)
            raise Drop(DROP_WRITE_ERROR)
        for k in range(min(self.len, new_len), self.stride):   # trimmed bytes are gone, grown ones zero
            self.b[k] = 0
        self.len = new_len


def _words(b):
    if len(b) & 1:
        b = b + b"\0"
    return struct.unpack(">%dH" % (len(b) // 2), b)


def csum_diff(frm, to):
    """bpf_csum_diff(from, to, seed 0) as a residue: sum(~from) + sum(to)."""
    return sum(0xffff - w for w in _words(frm)) + sum(_words(to))


def l4_csum_replace(skb, off, diff):
    if off + 2 > skb.len:
        raise Drop(DROP_CSUM_L4)
    old, = struct.unpack(">H", skb.load(off, 2))
    r = (diff + (0xffff - old) + 0xffff) % 0xffff
    if r == 0:
        r = 0xffff
    skb.store(off, struct.pack(">H", 0xffff - r))


def arp_respond(cfg, skb, mac):
    if skb.len < 14 + 8 + 20:
        return TC_OK
    b = skb.b
    dmac, smac = bytes(b[0:6]), bytes(b[6:12])
    ar_hrd, ar_op = bytes(b[14:16]), bytes(b[20:22])
    sip, tip = bytes(b[28:32]), bytes(b[38:42])
    if not (ar_op == b"\x00\x01" and ar_hrd == b"\x00\x01" and (dmac == b"\xff" * 6 or dmac == mac) and tip == cfg.gateway):
        return TC_OK
    skb.store(6, mac)
    skb.store(0, smac)
    skb.store(20, b"\x00\x02")
    skb.store(22, mac)
    skb.store(28, cfg.gateway)
    skb.store(32, smac)
    skb.store(38, sip)
    return TC_REDIRECT


def icmp6_send_reply(cfg, skb, mac):
    sip, dip = skb.load(22, 16), skb.load(38, 16)
    skb.store(22, cfg.router)
    skb.store(38, sip)
    l4_csum_replace(skb, 56, csum_diff(sip, cfg.router))
    l4_csum_replace(skb, 56, csum_diff(dip, sip))
    smac = skb.load(6, 6)
    skb.store(0, smac)
    skb.store(6, mac)
    return TC_REDIRECT


def send_echo_reply(cfg, skb, mac):
    old = skb.load(54, 8)
    new = bytes([129, 0]) + old[2:4] + old[4:8]
    skb.store(54, new)
    l4_csum_replace(skb, 56, csum_diff(old, new))
    return icmp6_send_reply(cfg, skb, mac)


def handle_ns(cfg, skb, mac):
    target = skb.load(62, 16)
    if target != cfg.router:
        if cfg.flags & F_NS_TO_STACK:
            return TC_OK
        raise Drop(DROP_UNKNOWN_TARGET)
    old = skb.load(54, 8)
    # icmp6_router | icmp6_solicited, override 0: the little-endian bitfield of linux/icmpv6.h puts
    # reserved:5 in bits 0-4, override bit 5, solicited bit 6, router bit 7 of the first byte
    new = bytes([136, 0]) + old[2:4] + bytes([(1 << 7) | (1 << 6), 0, 0, 0])
    skb.store(54, new)
    l4_csum_replace(skb, 56, csum_diff(old, new))
    opts_old = skb.load(78, 8)
    opts = bytes([2, 1]) + mac
    skb.store(78, opts)
    l4_csum_replace(skb, 56, csum_diff(opts_old, opts))
    return icmp6_send_reply(cfg, skb, mac)


def send_time_exceeded(cfg, skb, mac):
    ip6 = skb.load(14, 40)
    skb.store(20, bytes([58]))
    nh = ip6[6]
    if nh in (58, 17):
        un = 8
    elif nh == 6:
        un = 20
    else:
        raise Drop(DROP_UNKNOWN_L4)
    upper = skb.load(54, un)
    data = bytes([3, 0, 0, 0, 0, 0, 0, 0]) + ip6 + upper
    plen = len(data)
    # compute_icmp6_csum: the data, then the pseudo header with the original addresses
    s = sum(_words(data)) + sum(_words(ip6[8:40])) + sum(_words(struct.pack(">II", plen, 58)))
    trimlen = plen - struct.unpack(">H", ip6[4:6])[0]
    skb.change_tail(skb.len + trimlen, cfg.max_len)
    skb.store(54, data)
    skb.store(18, struct.pack(">H", plen))
    l4_csum_replace(skb, 56, s)
    return icmp6_send_reply(cfg, skb, mac)


CALLS = {CALL_ARP: arp_respond, CALL_NS: handle_ns, CALL_ECHO: send_echo_reply, CALL_TE: send_time_exceeded}


def respond(cfg, frames, lens, calls, lxc_id=None, flow_hash=None, snap_init=None):
    """gf_respond over a batch.  Returns (records, snap_out, events): snap_out starts as snap_init
    (rows of frames without a call, or with a missed tail call, keep it); events is the bytes of
    the drop records in batch order."""
    n, stride = frames.shape
    rec = np.zeros(n, RESP_OUT)
    snap = np.zeros_like(frames) if snap_init is None else snap_init.copy()
    events = []

    def drop_event(i, reason, source, length, row):
        cap = min(length, PAYLOAD)
        hdr = struct.pack("<BBHIIIIIII", 1, reason, source, 0 if flow_hash is None else int(flow_hash[i]), length, cap,
                          0, 0, 0, 0)
        pay = bytes(row[:min(cap, stride)]).ljust(PAYLOAD, b"\0")
        events.append(hdr + pay)

    for i in range(n):
        c, length = int(calls[i]), int(lens[i])
        rec[i]["call"], rec[i]["len"] = c, length
        if c == CALL_NONE:
            continue
        mac, source = cfg.node_mac, 0
        prog = None
        if lxc_id is not None:
            prog = cfg.progs.get(int(lxc_id[i]))
            if prog is not None:
                mac, source = prog[0], prog[1] & 0xffff
        if c > 4 or (lxc_id is not None and prog is None):
            rec[i]["action"], rec[i]["reason"] = TC_SHOT, DROP_MISSED_TAIL_CALL
            drop_event(i, DROP_MISSED_TAIL_CALL, source, length, frames[i])
            continue
        skb = Skb(bytes(frames[i]), length, stride)
        try:
            rec[i]["action"] = CALLS[c](cfg, skb, mac)
        except Drop as d:
            rec[i]["action"], rec[i]["reason"] = TC_SHOT, d.reason
            drop_event(i, d.reason, source, skb.len, skb.b)
        rec[i]["len"] = skb.len
        snap[i] = np.frombuffer(bytes(skb.b), np.uint8)
    return rec, snap, events


# ---------------------------------------------------------------- an independent check
def icmp6_checksum_ok(row):
    """From scratch: the one's-complement sum of the IPv6 pseudo header and the ICMPv6 message of
    a fully captured frame, checksum field included, is 0 (0xffff)."""
    row = bytes(row)
    plen, = struct.unpack(">H", row[18:20])
    msg = row[54:54 + plen]
    s = sum(_words(row[22:54])) + sum(_words(struct.pack(">II", plen, 58))) + sum(_words(msg))
    while s >> 16:
        s = (s & 0xffff) + (s >> 16)
    return s == 0xffff


def icmp6_fill_checksum(fr):
    """Sets a valid ICMPv6 checksum in a fully captured frame (bytearray)."""
    fr[56:58] = b"\0\0"
    plen, = struct.unpack(">H", bytes(fr[18:20]))
    s = sum(_words(bytes(fr[22:54]))) + sum(_words(struct.pack(">II", plen, 58))) + sum(_words(bytes(fr[54:54 + plen])))
    while s >> 16:
        s = (s & 0xffff) + (s >> 16)
    fr[56:58] = struct.pack(">H", 0xffff - s)


# ---------------------------------------------------------------- frames
def eth(dmac, smac, ethertype):
    return bytes(dmac) + bytes(smac) + struct.pack(">H", ethertype)


def arp_frame(dmac, smac, op, sip, tip, hrd=1, pad=0):
    return eth(dmac, smac, 0x0806) + struct.pack(">HHBBH", hrd, 0x0800, 6, 4, op) + bytes(smac) + bytes(sip) + \
        bytes(6) + bytes(tip) + bytes(pad)


def ip6_frame(dmac, smac, saddr, daddr, nexthdr, payload, hop=64, payload_len=None):
    pl = len(payload) if payload_len is None else payload_len
    return eth(dmac, smac, 0x86DD) + struct.pack(">IHBB", 6 << 28, pl, nexthdr, hop) + bytes(saddr) + bytes(daddr) + \
        bytes(payload)


def ns_frame(dmac, smac, saddr, daddr, target, opt=True):
    body = bytes([135, 0, 0, 0, 0, 0, 0, 0]) + bytes(target) + (bytes([1, 1]) + bytes(smac) if opt else b"")
    fr = bytearray(ip6_frame(dmac, smac, saddr, daddr, 58, body, hop=255))
    icmp6_fill_checksum(fr)
    return bytes(fr)


def echo_frame(dmac, smac, saddr, daddr, ident, seq, data):
    body = bytes([128, 0, 0, 0]) + struct.pack(">HH", ident, seq) + bytes(data)
    fr = bytearray(ip6_frame(dmac, smac, saddr, daddr, 58, body))
    icmp6_fill_checksum(fr)
    return bytes(fr)


GATEWAY = bytes([10, 11, 0, 1])
ROUTER = bytes.fromhex("f00d0000000000000000000000010000")
NODE_MAC = bytes.fromhex("deadbeefc0de")
PROGS = {3000 + k: (bytes.fromhex("bb22222222%02x" % k), 3000 + k) for k in range(6)}
EMPTY_SLOT = 3100


def default_cfg(flags=0, max_len=0):
    return Cfg(GATEWAY, ROUTER, NODE_MAC, PROGS, flags, max_len)


def fuzz(seed, n, stride, with_lxc=True):
    """n responder frames: (frames [n,stride], lens, calls, lxc_id or None, flow_hash).  About a sixth
    of the frames have no call; the rest are ARP, NS, echo requests and hop-limit-expired IPv6
    frames, well-formed and broken, plus call values above 4 and (with_lxc) empty slots."""
    rng = np.random.default_rng(seed)
    frames, lens = np.zeros((n, stride), np.uint8), np.zeros(n, np.uint32)
    calls = np.zeros(n, np.uint8)
    lxc = np.zeros(n, np.uint16)
    rb = lambda k: bytes(rng.integers(0, 256, k, dtype=np.uint8))
    pod6 = lambda: bytes.fromhex("f00d000000000000000000000a0b") + rb(2)
    for i in range(n):
        lid = 3000 + int(rng.integers(0, 6))
        if with_lxc and rng.random() < 0.04:
            lid = EMPTY_SLOT + int(rng.integers(0, 4))
        lxc[i] = lid
        mac = PROGS[lid][0] if with_lxc and lid in PROGS else NODE_MAC
        smac = b"\xaa" + rb(5)
        kind = rng.random()
        v = rng.random()
        length = None
        if kind < 0.15:
            c, fr = CALL_NONE, rb(int(rng.integers(14, 200)))
        elif kind < 0.36:
            c = CALL_ARP
            dmac = b"\xff" * 6 if v < 0.45 else mac if v < 0.8 else b"\x02" + rb(5)
            v2 = rng.random()
            tip = GATEWAY if v2 < 0.75 else bytes([10, 11, 0, 2])
            v3 = rng.random()
            op, hrd = (2 if v3 < 0.1 else 1), (6 if 0.1 <= v3 < 0.17 else 1)
            fr = arp_frame(dmac, smac, op, bytes([10, 11, 0, 7]) + b"", tip, hrd, pad=int(rng.integers(0, 19)))
            if rng.random() < 0.08:
                length = int(rng.integers(14, 42))
        elif kind < 0.56:
            c = CALL_NS
            target = ROUTER if v < 0.6 else pod6()
            fr = ns_frame(b"\x33\x33\xff" + target[13:], smac, pod6(), b"\xff\x02" + bytes(9) + b"\x01\xff" + target[13:], target,
                          opt=rng.random() < 0.85)
            v2 = rng.random()
            if v2 < 0.08:
                length = int(rng.integers(54, 78))
            elif v2 < 0.16:
                length = int(rng.integers(78, 86))
        elif kind < 0.74:
            c = CALL_ECHO
            fr = bytearray(echo_frame(mac, smac, pod6(), ROUTER, int(rng.integers(0, 65536)), int(rng.integers(0, 65536)),
                                      rb(int(rng.integers(0, stride - 62 + 1)))))
            if v < 0.1:
                fr[56] ^= 0x5a                         # a wrong request checksum stays wrong
            fr = bytes(fr)
            if 0.1 <= v < 0.2:
                length = int(rng.integers(54, 62))
        elif kind < 0.95:
            c = CALL_TE
            nh = 17 if v < 0.3 else 6 if v < 0.6 else 58 if v < 0.8 else int(rng.choice([0, 43, 44, 50, 132]))
            un = 20 if nh == 6 else 8
            body = rb(un + int(rng.integers(0, 40)))
            pl = None
            v2 = rng.random()
            if v2 < 0.08:
                body = rb(int(rng.integers(0, un)))     # the upper header is cut short
            elif v2 < 0.16:
                pl = int(rng.integers(0, 65536))         # payload_len unrelated to the frame
            fr = ip6_frame(mac, smac, pod6(), bytes.fromhex("f00d00000000000000000000c0a8") + rb(2), nh, body,
                           hop=int(rng.integers(0, 2)), payload_len=pl)
            if 0.16 <= v2 < 0.26:
                fr += bytes(int(rng.integers(1, 12)))    # trailing padding
            elif 0.26 <= v2 < 0.34:
                length = int(rng.integers(1400, 1600))   # a long frame, captured in part
        else:
            c, fr = int(rng.integers(5, 256)), echo_frame(mac, smac, pod6(), ROUTER, 1, 1, b"")
        fr = fr[:stride] if length is None else fr
        lens[i] = len(fr) if length is None else length
        if length is None and c == CALL_TE and len(fr) == stride and rng.random() < 0.5:
            lens[i] = stride + int(rng.integers(0, 400))   # more on the wire than in the snap
        fr = fr[:stride]
        frames[i, :len(fr)] = np.frombuffer(fr, np.uint8)
        calls[i] = c
    fh = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    return frames, lens, calls, (lxc if with_lxc else None), fh
