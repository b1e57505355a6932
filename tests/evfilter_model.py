"""A restatement of `cilium monitor`'s filter and of gf_event_drain's output rules, the checker
of tests/test_event_filter.py and tests/test_gpu_event_filter.py.

The filter (cilium/cmd/monitor.go):
  :144-156  match(messageType, src, dst): each of --type, --from, --to, --related-to applies only
            when given (len > 0); --related-to passes on either side
  :165      dropEvents     match(MessageTypeDrop,    dn.Source, uint16(dn.DstID))
  :182      traceEvents    match(MessageTypeTrace,   tn.Source, tn.DstID)
  :199      debugEvents    match(MessageTypeDebug,   dm.Source, 0)
  :215      captureEvents  match(MessageTypeCapture, dc.Source, 0)
  pkg/monitor/types.go:29-33  MessageTypeDrop 1, Debug 2, Capture 3, Trace 4
The layouts (little-endian, as the ring holds them):
  pkg/monitor/datapath_drop.go   DropNotify   Type u8, SubType u8, Source u16, Hash u32, OrigLen u32,
                                              CapLen u32, SrcLabel u32, DstLabel u32, DstID u32 (byte 24), Ifindex u32
  pkg/monitor/datapath_trace.go  TraceNotify  the same up to DstLabel, then DstID u16 (byte 24), Reason u8, Pad u8, Ifindex u32
  pkg/monitor/datapath_debug.go  DebugMsg     Type, SubType, Source u16, Hash u32, Arg1..3 u32 (20 B)
                                 DebugCapture Type, SubType, Source u16, Hash u32, two u32 lengths, Arg1, Arg2 u32 (24 B);
                                              the datapath writes len_orig at byte 8 and len_cap at byte 12
                                              (bpf/lib/dbg.h:183-189), as drop and trace records have them
So in the three layouts with a payload the u32 at byte 12 is the captured length that follows the
header; a DebugMsg has none.
"""
import struct

import numpy as np

SLOT = 160
DROP, DEBUG, CAPTURE, TRACE = 1, 2, 3, 4
HDR = {DROP: 32, DEBUG: 20, CAPTURE: 24, TRACE: 32}


# ---------------------------------------------------------------- one record
def slot(type, source, dst_id=0, len_cap=0, junk24=None, fill=0xAB):
    """One ring slot from its fields; the bytes past the header are `fill` (a real ring holds the
    payload, then zeros), junk24: two bytes to put at offset 24 of a debug or capture record."""
    b = bytearray([fill]) * SLOT
    if type == DROP:
        b[:32] = struct.pack("<BBHIIIIIII", type, 130, source, 0x11223344, 200, len_cap, 300, 400, dst_id, 11)
    elif type == TRACE:
        b[:32] = struct.pack("<BBHIIIIIHBBI", type, 0, source, 0x11223344, 200, len_cap, 300, 400, dst_id, 2, 0, 11)
    elif type == DEBUG:
        b[:20] = struct.pack("<BBHIIII", type, 6, source, 0x11223344, 1, 2, 3)
    elif type == CAPTURE:
        b[:24] = struct.pack("<BBHIIIII", type, 4, source, 0x11223344, 200, len_cap, 1, 2)
    else:                                   # an unknown type: a header-shaped record all the same
        b[:32] = struct.pack("<BBHIIIIIII", type, 0, source, 0, 0, len_cap, 0, 0, dst_id, 0)
    if junk24 is not None:
        b[24:26] = struct.pack("<H", junk24)
    return bytes(b)


def endpoints(rec):
    """(type, src, dst) of one slot as the handlers pass them to match."""
    b = bytes(rec[:28])
    t, src = b[0], struct.unpack_from("<H", b, 2)[0]
    if t == DROP:
        dst = struct.unpack_from("<I", b, 24)[0] & 0xffff       # uint16(dn.DstID)
    elif t == TRACE:
        dst = struct.unpack_from("<H", b, 24)[0]
    else:
        dst = 0
    return t, src, dst


def match_one(rec, types=(), frm=(), to=(), related=()):
    t, src, dst = endpoints(rec)
    if t not in HDR:
        return False                        # "Unknown event": printed whatever the filter, never a match
    if len(types) > 0 and t not in types:
        return False
    elif len(frm) > 0 and src not in frm:
        return False
    elif len(to) > 0 and dst not in to:
        return False
    elif len(related) > 0 and src not in related and dst not in related:
        return False
    return True


def wire_len(rec):
    """The bytes of a record on the wire (GF_EVD_F_PACKED): header + len_cap, clamped to the slot."""
    b = bytes(rec[:16])
    t = b[0]
    cap = 0 if t == DEBUG else struct.unpack_from("<I", b, 12)[0]
    return min(HDR[t] + cap, SLOT)


# ---------------------------------------------------------------- a whole drain, in numpy
def select(ring, types=(), frm=(), to=(), related=()):
    """(match, known) boolean columns over a [n, 160] uint8 ring."""
    ring = np.ascontiguousarray(ring, np.uint8).reshape(-1, SLOT)
    t = ring[:, 0]
    src = ring[:, 2:4].copy().view("<u2")[:, 0]
    d16 = ring[:, 24:26].copy().view("<u2")[:, 0]
    dst = np.where((t == DROP) | (t == TRACE), d16, 0)
    known = (t >= 1) & (t <= 4)
    m = known.copy()
    if len(types):
        m &= np.isin(t, list(types))
    if len(frm):
        m &= np.isin(src, list(frm))
    if len(to):
        m &= np.isin(dst, list(to))
    if len(related):
        m &= np.isin(src, list(related)) | np.isin(dst, list(related))
    return m, known


def wire_lens(ring):
    ring = np.ascontiguousarray(ring, np.uint8).reshape(-1, SLOT)
    t = ring[:, 0].astype(np.int64)
    cap = ring[:, 12:16].copy().view("<u4")[:, 0].astype(np.int64)
    cap = np.where(t == DEBUG, 0, cap)
    hdr = np.select([t == DEBUG, t == CAPTURE], [20, 24], 32)
    return np.minimum(hdr + cap, SLOT)


MAX_WINDOW = 1 << 24


def drain(ring, count, capacity=None, first=0, max_n=0, packed=False, out_bytes=None, **filt):
    """gf_event_drain over `ring` ([capacity, 160] uint8) holding `count` (which may exceed the
    capacity: the overrun).  Returns a dict: every field of gf_event_drain_out, `out` (the bytes
    stored, res.bytes of them) and `off` (written + 1 offsets)."""
    ring = np.ascontiguousarray(ring, np.uint8).reshape(-1, SLOT)
    capacity = len(ring) if capacity is None else capacity
    end = min(count, capacity, first + (max_n or MAX_WINDOW))
    lo = min(first, end)
    win = ring[lo:end]
    m, known = select(win, **filt)
    idx = np.flatnonzero(m)
    wire = wire_lens(win[idx]) if packed else np.full(len(idx), SLOT, np.int64)
    take = (wire + 7) // 8 * 8 if packed else wire
    ends = np.cumsum(take)
    if out_bytes is None:
        out_bytes = int(ends[-1]) if len(ends) else 0
    written = int(np.searchsorted(ends, out_bytes, side="right"))     # the prefix whose running total fits
    off = np.concatenate([[0], ends[:written]]).astype(np.int64)
    rows = win[idx[:written]].copy()
    col = np.arange(SLOT)[None, :]
    rows[col >= wire[:written, None]] = 0                              # the padding up to a multiple of 8
    out = rows[col < take[:written, None]]
    t = win[:, 0]
    return dict(count=count, lost=max(count, capacity) - capacity, seen=end - lo, matched=len(idx), written=written,
                unknown=int((~known).sum()), bytes=int(off[-1]),
                by_type=[0] + [int((m & (t == k)).sum()) for k in (1, 2, 3, 4)],
                out=out.tobytes(), off=[int(x) for x in off], index=[int(x) + lo for x in idx])


# ---------------------------------------------------------------- synthetic rings
IDS = np.array([0, 65535, 5, 7, 9, 100, 2000, 40000], np.uint16)
LEN_CAPS = np.array([0, 1, 7, 8, 64, 127, 128, 200], np.uint32)       # 200: past the slot, the clamp


def synth_ring(n, seed=1, unknown=0.02):
    """n slots of random bytes (so that a packed drain has non-zero bytes to leave out) with the
    fields the drain reads set: all four types plus about 2 % unknown ones, source and
    destination from IDS, len_cap from LEN_CAPS; the upper half of a drop record's DstID stays
    random (the truncation)."""
    rng = np.random.default_rng(seed)
    ring = rng.integers(0, 256, (n, SLOT), dtype=np.uint8)
    t = rng.integers(1, 5, n).astype(np.uint8)
    bad = rng.random(n) < unknown
    t[bad] = rng.choice(np.array([0, 5, 9, 129, 255], np.uint8), int(bad.sum()))
    ring[:, 0] = t
    ring[:, 2:4] = IDS[rng.integers(0, len(IDS), n)].view(np.uint8).reshape(n, 2)
    ring[:, 12:16] = LEN_CAPS[rng.integers(0, len(LEN_CAPS), n)].view(np.uint8).reshape(n, 4)
    ring[:, 24:26] = IDS[rng.integers(0, len(IDS), n)].view(np.uint8).reshape(n, 2)
    return ring
