"""cilium monitor's filters (gf_event_filter_load / gf_event_drain) without a GPU: the model of
tests/evfilter_model.py against hand-derived cases, cilium_amd.monitor.match against the model,
the struct layouts, and every refusal of the two calls (all of them precede any launch)."""
import ctypes as C
import errno
import json
import os

import numpy as np
import pytest

from cilium_amd import monitor as MON
from cilium_amd._lib import (lib, gf_event_ring, gf_event_filter_cfg, gf_event_drain_out, GF_EVF_MAX_IDS,
                             GF_EVD_F_PACKED, GF_EVD_F_RESET, GF_EVD_MAX_WINDOW)
from tests import evfilter_model as M

KATS = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "evfilter_kats.json")))


def kat_ring():
    return np.frombuffer(b"".join(M.slot(**{k: v for k, v in r.items() if k != "note"}) for r in KATS["ring"]),
                         np.uint8).reshape(-1, M.SLOT)


@pytest.mark.parametrize("case", KATS["cases"], ids=lambda c: c["name"])
def test_model_against_the_kats(case):
    ring = kat_ring()
    assert len(ring) == 12
    got = [k for k in range(len(ring)) if M.match_one(ring[k], **case["filter"])]
    assert got == case["index"]
    for packed in (False, True):
        d = M.drain(ring, len(ring), packed=packed, **case["filter"])
        assert d["index"] == case["index"] and d["unknown"] == KATS["unknown"] and d["matched"] == len(got)
        assert d["written"] == len(got) and d["seen"] == 12 and d["lost"] == 0
        assert sum(d["by_type"]) == len(got) and d["by_type"][0] == 0
        want = [KATS["packed_wire_len"][k] if packed else 160 for k in got]
        assert [b - a for a, b in zip(d["off"][:-1], d["off"][1:])] == [(w + 7) // 8 * 8 for w in want]
        for k, a, w in zip(got, d["off"], want):
            rec = d["out"][a:a + (w + 7) // 8 * 8]
            assert rec[:w] == ring[k].tobytes()[:w] and not any(rec[w:])
    dec = MON.decode_packed(np.frombuffer(d["out"], np.uint8), d["off"])       # the packed drain, decoded
    assert len(dec) == len(got)
    for k, e in zip(got, dec):
        whole, w = MON.decode(ring[k]), KATS["packed_wire_len"][k]
        assert {f: v for f, v in e.items() if f != "data"} == {f: v for f, v in whole.items() if f != "data"}
        if "data" in whole:
            assert e["data"] == ring[k].tobytes()[M.HDR[e["type"]]:w].ljust(len(e["data"]), b"\0")


def test_kat_wire_lengths():
    ring = kat_ring()
    for k, w in enumerate(KATS["packed_wire_len"]):
        if w is not None:
            assert M.wire_len(ring[k]) == w
    assert list(M.wire_lens(ring[[0, 1, 2, 3, 4, 5, 8, 9, 10, 11]])) == [w for w in KATS["packed_wire_len"] if w is not None]


FILTERS = [dict(), dict(types=(1, 4)), dict(frm=(5, 0)), dict(to=(0,)), dict(to=(65535, 7)), dict(related=(9,)),
           dict(types=(2, 3, 4), frm=(5, 7, 9), to=(0, 5), related=(5, 100)), dict(frm=(1234,)),
           dict(types=(1, 2, 3, 4), related=tuple(int(x) for x in M.IDS))]


@pytest.mark.parametrize("filt", FILTERS, ids=lambda f: "-".join(f) or "none")
def test_monitor_match_and_numpy_model_against_the_per_record_model(filt):
    ring = M.synth_ring(3000, seed=5)
    want = [M.match_one(r, **filt) for r in ring]
    assert [MON.match(r, **filt) for r in ring] == want
    assert [MON.match(MON.decode(r), **filt) for r in ring] == want          # over decoded records too
    m, known = M.select(ring, **filt)
    assert list(m) == want and list(known) == [1 <= r[0] <= 4 for r in ring]
    if filt:
        assert any(want) != (filt == dict(frm=(1234,))) and not all(want)


def test_model_output_cut_and_window():
    ring = M.synth_ring(300, seed=6)
    full = M.drain(ring, 300, packed=True)
    cut = M.drain(ring, 300, packed=True, out_bytes=full["off"][40] + 7)     # 7 bytes short of the 41st... of none
    assert cut["written"] == 40 and cut["bytes"] == full["off"][40] and cut["out"] == full["out"][:cut["bytes"]]
    assert cut["matched"] == full["matched"]
    slot = M.drain(ring, 300, out_bytes=160 * 3 + 159)
    assert slot["written"] == 3 and slot["off"] == [0, 160, 320, 480]
    over = M.drain(ring[:100], 300)
    assert (over["count"], over["lost"], over["seen"]) == (300, 200, 100)
    mid = M.drain(ring, 250, first=100, max_n=50)
    assert mid["seen"] == 50 and mid["index"] == [k for k in full["index"] if 100 <= k < 150]
    assert M.drain(ring, 250, first=250)["seen"] == 0 and M.drain(ring, 250, first=4000)["seen"] == 0


def test_struct_layouts():
    assert C.sizeof(gf_event_filter_cfg) == 56 and C.sizeof(gf_event_drain_out) == 56
    assert gf_event_drain_out.bytes.offset == 24 and gf_event_drain_out.by_type.offset == 32
    assert gf_event_filter_cfg.to.offset == 24 and gf_event_filter_cfg.n_related.offset == 48


# ---------------------------------------------------------------- refusals
def _cfg(mask=0, frm=(), to=(), related=()):
    arr = [(C.c_uint16 * max(len(x), 1))(*x) for x in (frm, to, related)]
    return gf_event_filter_cfg(mask, arr[0], len(frm), arr[1], len(to), arr[2], len(related))


def test_filter_load_refusals_and_close():
    assert lib.gf_event_filter_load(None) == -errno.EFAULT
    for field in ("n_from", "n_to", "n_related"):
        cfg = gf_event_filter_cfg()
        setattr(cfg, field, 1)                                               # a NULL list with n != 0
        assert lib.gf_event_filter_load(C.byref(cfg)) == -errno.EFAULT
    for mask in (1, 1 << 5, 0x80000000, 0x1f):
        assert lib.gf_event_filter_load(C.byref(_cfg(mask))) == -errno.EINVAL
    big = (C.c_uint16 * (GF_EVF_MAX_IDS + 1))()
    for field, n in (("frm", "n_from"), ("to", "n_to"), ("related", "n_related")):
        cfg = gf_event_filter_cfg()
        setattr(cfg, field, big)
        setattr(cfg, n, GF_EVF_MAX_IDS + 1)
        assert lib.gf_event_filter_load(C.byref(cfg)) == -errno.E2BIG
        setattr(cfg, n, GF_EVF_MAX_IDS)                                      # the longest list loads
        h = lib.gf_event_filter_load(C.byref(cfg))
        assert h > 0 and lib.gf_obj_close(h) == 0
    h = lib.gf_event_filter_load(C.byref(_cfg(0x1e, (0, 65535), (5,), (7, 7))))
    assert h > 0
    assert lib.gf_obj_close(h) == 0
    assert lib.gf_obj_close(h) == -errno.EBADF                               # gone
    ring = gf_event_ring(0x1000, 4, 0x2000)
    assert lib.gf_event_drain(h, C.byref(ring), 0, 0, 0, None, 0, None, 0x3000, None) == -errno.EBADF


def test_event_filter_class():
    f = MON.EventFilter(types=(1, 4), frm=(5,))
    assert f.handle > 0 and f.match(M.slot(1, 5)) and not f.match(M.slot(2, 5)) and not f.match(M.slot(4, 6))
    f.close()
    assert f.handle == 0
    with pytest.raises(OSError):
        MON.EventFilter(types=(7,))


def test_drain_refusals():
    """Addresses that are never dereferenced: every refusal precedes any launch."""
    from cilium_amd import bpf
    filt = lib.gf_event_filter_load(C.byref(_cfg()))
    assert filt > 0
    RECS, CNT, RES, OUT = 0x100000, 0x200000, 0x300000, 0x400000
    ring = gf_event_ring(RECS, 1024, CNT)
    call = lambda h=filt, r=ring, first=0, max_n=0, flags=0, out=OUT, nb=160, off=None, res=RES: lib.gf_event_drain(
        h, C.byref(r) if r is not None else None, first, max_n, flags, out, nb, off, res, None)
    m = bpf.CreateMap(1, 4, 4, 16, 0)                                         # a handle of another kind
    assert call(h=m) == -errno.EBADF and call(h=0) == -errno.EBADF and call(h=1 << 20) == -errno.EBADF
    bpf.ObjClose(m)
    assert call(r=None) == -errno.EFAULT
    assert call(r=gf_event_ring(None, 1024, CNT)) == -errno.EFAULT
    assert call(r=gf_event_ring(RECS, 1024, None)) == -errno.EFAULT
    assert call(res=None) == -errno.EFAULT
    assert call(out=None, nb=160) == -errno.EFAULT
    assert call(flags=4) == -errno.EINVAL and call(flags=GF_EVD_F_PACKED | GF_EVD_F_RESET | 0x100) == -errno.EINVAL
    for out, nb in ((RECS, 160), (RECS + 1024 * 160 - 1, 1), (RECS - 100, 101), (RECS - 100, 1 << 30), (RECS + 320, 16)):
        assert call(out=out, nb=nb) == -errno.EINVAL, (out, nb)              # out overlaps the ring's records
    assert call(r=gf_event_ring(RECS + 2, 1024, CNT)) == -errno.EINVAL        # records not 4-byte aligned
    assert call(max_n=GF_EVD_MAX_WINDOW + 1) == -errno.E2BIG
    assert lib.gf_obj_close(filt) == 0
