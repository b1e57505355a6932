"""Geneve option TLVs as the agent handles them (pkg/geneve/geneve.go) and the option
buffer an endpoint's from-container program sends (GENEVE_OPTS, pkg/endpoint/bpf.go:375-394).

The agent keeps an endpoint's options as `class;type;len;hexdata` lines (WriteOpts) and turns
them into the raw bytes of the C initialiser with ReadOpts: class as a big-endian u16, the
type byte, `len >> 2` in the fourth byte (the Geneve length field counts 4-byte words; its
three upper bits are reserved) and the data.  bpf/lib/geneve.h:46-60 is the receiving side.
"""
from dataclasses import dataclass

GENEVE_CLASS_EXPERIMENTAL = 0xffff   # bpf/lib/geneve.h:22
GENEVE_TYPE_SECLABEL = 1             # bpf/lib/geneve.h:23
MAX_GENEVE_OPT_LEN = 64              # bpf/lib/geneve.h:21: the receive buffer


@dataclass
class GeneveTlv:
    """GeneveTlv (geneve.go:26-31); opt_len is the data length in bytes."""
    opt_class: int
    opt_type: int
    opt_len: int
    opt_data: bytes = b""


def validate(tlv):
    """ValidateOpt (geneve.go:33-39): sz > 124, sz % 4 != 0 and sz != len(data) fail."""
    sz = tlv.opt_len
    return not (sz > 124 or sz % 4 != 0 or sz != len(tlv.opt_data))


def _uint(text, bits, hex_fallback=False):
    """strconv.ParseUint(text, 0, bits) with the error dropped as ReadOpts drops it (0).
    hex_fallback: a class written without its 0x prefix (`ffff`) is read as hexadecimal."""
    try:
        v = int(text.strip(), 0)
    except ValueError:
        try:
            v = int(text.strip(), 16) if hex_fallback else 0
        except ValueError:
            v = 0
    return v if 0 <= v < (1 << bits) else 0


def format_line(opt_class, opt_type, opt_len, data):
    """One line as WriteOpts writes it (geneve.go:84-97); data: bytes or a hex string."""
    hx = data if isinstance(data, str) else bytes(data).hex()
    return f"{opt_class};{opt_type};{opt_len};{hx}\n"


def encode(text):
    """ReadOpts (geneve.go:41-82) over the file's text: returns (TLVs, raw bytes).  Raises
    ValueError where ReadOpts returns an error: a line without four fields, or a TLV that
    fails validate()."""
    tlvs, raw = [], bytearray()
    for k, line in enumerate(l for l in text.splitlines() if l.strip()):
        rec = line.split(";")
        if len(rec) != 4:
            raise ValueError(f"Geneve tlv {k}: expected class;type;len;hexdata, got {line!r}")
        try:
            data = bytes.fromhex(rec[3].strip())
        except ValueError:
            data = b""                                  # hex.DecodeString's error is dropped too
        tlv = GeneveTlv(_uint(rec[0], 16, True), _uint(rec[1], 8), _uint(rec[2], 8), data)
        raw += bytes([tlv.opt_class >> 8, tlv.opt_class & 0xff, tlv.opt_type, tlv.opt_len >> 2]) + data
        if not validate(tlv):
            raise ValueError(f"Geneve tlv {k} validation failed {tlv.opt_class:x} {tlv.opt_type:x} {tlv.opt_len:x}")
        tlvs.append(tlv)
    return tlvs, bytes(raw)


def decode(raw):
    """The TLVs of a raw option buffer (the inverse of encode's bytes): the length field's low
    five bits count 4-byte words, the reserved bits are ignored.  Raises ValueError for a
    buffer that ends inside a TLV."""
    raw, tlvs, off = bytes(raw), [], 0
    while off < len(raw):
        if off + 4 > len(raw):
            raise ValueError(f"truncated Geneve option header at byte {off}")
        sz = (raw[off + 3] & 0x1f) << 2
        if off + 4 + sz > len(raw):
            raise ValueError(f"truncated Geneve option data at byte {off}")
        tlvs.append(GeneveTlv((raw[off] << 8) | raw[off + 1], raw[off + 2], sz, raw[off + 4:off + 4 + sz]))
        off += 4 + sz
    return tlvs


def lines(tlvs):
    """The TLVs as the lines writeGeneve passes to WriteOpts (`0xffff;0x1;4;0000011e`)."""
    return "".join(format_line(hex(t.opt_class), hex(t.opt_type), t.opt_len, t.opt_data) for t in tlvs)


def endpoint_opts(identity):
    """writeGeneve (pkg/endpoint/bpf.go:375-394): the 8 bytes of an endpoint's GENEVE_OPTS —
    class 0xffff, type 1, length 4 and the identity as a big-endian u32."""
    _, raw = encode(format_line("0xffff", "0x1", "4", f"{identity & 0xffffffff:08x}"))
    return raw
