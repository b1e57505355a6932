"""gf_event_drain on the GPU (k_evd_count, k_evd_scan, k_evd_scatter) against the numpy model of
tests/evfilter_model.py: every byte of out, every offset and every field of the result, over
synthetic rings (all four record types, unknown types, random bytes past the wire length) and
over the ring one ingress call leaves."""

import numpy as np
import pytest

from cilium_amd import monitor as MON
from cilium_amd import synth
from tests import evfilter_model as M

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

FILTERS = {
    "none": dict(),
    "type": dict(types=(1, 4)),
    "from": dict(frm=(5, 0)),
    "to": dict(to=(0, 65535)),
    "related": dict(related=(9, 7)),
    "all": dict(types=(2, 3, 4), frm=(5, 7, 9, 65535), to=(0, 5, 7), related=(5, 100, 0)),
    "nothing": dict(frm=(1234,)),
    "everything": dict(types=(1, 2, 3, 4), related=tuple(int(x) for x in M.IDS)),
}
SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 3 * 256 + 1, 70001]
POISON = 0x5A
RING = M.synth_ring(70001, seed=11)          # every size is a prefix of this one
FIELDS = ("count", "lost", "seen", "matched", "written", "unknown", "bytes", "by_type")


@pytest.fixture(scope="module")
def dp():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(0)
    from cilium_amd.datapath import Datapath
    d = Datapath(synth.Scenario("evfilter"), pin_prefix=None)
    yield d
    d.close()


@pytest.fixture(scope="module")
def filters(dp):
    fs = {k: MON.EventFilter(**v) for k, v in FILTERS.items()}
    yield fs
    for f in fs.values():
        f.close()


def load(dp, ring, count, capacity=None):
    """A ring of `capacity` slots holding `ring`'s rows, with the count word set."""
    capacity = len(ring) if capacity is None else capacity
    recs, cnt, _ = dp.set_event_ring(capacity)
    if capacity:
        recs[:capacity].copy_(torch.from_numpy(np.ascontiguousarray(ring[:capacity])))
    cnt.fill_(count)
    return recs, cnt


def check(dp, f, ring, count, what, capacity=None, first=0, max_n=0, packed=False, out_bytes=None, shift=0):
    """One drain against the model: res, out (with the bytes past res.bytes untouched) and out_off."""
    capacity = len(ring) if capacity is None else capacity
    want = M.drain(ring[:capacity], count, capacity, first, max_n, packed, out_bytes, **FILTERS[f[0]])
    room = want["bytes"] + 64 if out_bytes is None else out_bytes
    buf = torch.full((room + 64 + shift,), POISON, dtype=torch.uint8, device="cuda")
    out = buf[shift:shift + room] if out_bytes is not None else buf[shift:]
    _, off, res = dp.event_drain(f[1], first=first, max_n=max_n, packed=packed, out_records=out)
    for k in FIELDS:
        assert res[k] == want[k], (what, k, res[k], want[k])
    got = buf.cpu().numpy()
    assert got[shift:shift + want["bytes"]].tobytes() == want["out"], (what, "out")
    assert (got[:shift] == POISON).all() and (got[shift + want["bytes"]:] == POISON).all(), (what, "past the output")
    assert off[:want["written"] + 1].cpu().numpy().tolist() == want["off"], (what, "out_off")
    return want


@pytest.mark.parametrize("n", SIZES)
def test_sizes_filters_and_modes(dp, filters, n):
    """Block and wave boundaries (63..257, 3 * 256 + 1) and a ring of 274 blocks, whose block sums
    the scan's lanes and waves share; every filter in both modes."""
    load(dp, RING[:n], n)
    seen = set()
    for name, f in filters.items():
        for packed in (False, True):
            w = check(dp, (name, f), RING[:n], n, (n, name, packed), packed=packed)
            seen.add((w["matched"] == 0, w["matched"] == n - w["unknown"]))
    if n >= 255:
        assert seen == {(True, False), (False, True), (False, False)}      # nothing, everything and a part were all seen


def test_overrun_and_window(dp, filters):
    ring, f = RING[:1000], ("type", filters["type"])
    load(dp, ring, 5000, capacity=600)                                      # the ring overran: 4400 lost, 600 to see
    w = check(dp, f, ring, 5000, "overrun", capacity=600)
    assert (w["lost"], w["seen"]) == (4400, 600)
    load(dp, ring, 900)
    for packed in (False, True):
        w = check(dp, f, ring, 900, "first in the middle", first=301, packed=packed)
        assert w["seen"] == 599
        w = check(dp, f, ring, 900, "max_n cuts", first=130, max_n=300, packed=packed)
        assert w["seen"] == 300 and w["index"][-1] < 430
        w = check(dp, f, ring, 900, "max_n past the end", first=700, max_n=5000, packed=packed)
        assert w["seen"] == 200
        for first in (900, 901, 1000, 4000):
            w = check(dp, f, ring, 900, "first past the end", first=first, packed=packed)
            assert (w["seen"], w["matched"], w["count"]) == (0, 0, 900)


def test_output_cut(dp, filters):
    """out_bytes smaller than the matches: a prefix is written, nothing past res.bytes; the cut
    falls in the first block, in a middle one, on a record boundary and at 0."""
    ring, f = RING[:2000], ("from", filters["from"])
    load(dp, ring, 2000)
    for packed in (False, True):
        full = M.drain(ring, 2000, packed=packed, **FILTERS["from"])
        assert full["matched"] > 300
        for k in (1, 37, 300):
            for extra in (0, 7):
                w = check(dp, f, ring, 2000, ("cut", packed, k), packed=packed, out_bytes=full["off"][k] + extra)
                assert w["written"] == k < w["matched"] and w["bytes"] == full["off"][k]
        w = check(dp, f, ring, 2000, ("cut", packed, 0), packed=packed, out_bytes=0)
        assert w["written"] == 0 and w["matched"] == full["matched"]
        w = check(dp, f, ring, 2000, ("cut", packed, "7 bytes"), packed=packed, out_bytes=7)
        assert w["written"] == 0


def test_unaligned_out(dp, filters):
    """out at odd addresses: the byte-copy kernels give the same bytes."""
    ring = RING[:777]
    load(dp, ring, 777)
    for shift in (1, 4, 8):
        for packed in (True, False):
            check(dp, ("all", filters["all"]), ring, 777, ("shift", shift, packed), packed=packed, shift=shift)
            check(dp, ("none", filters["none"]), ring, 777, ("shift", shift, packed), packed=packed, shift=shift)


def _real(dp_real, sc, fresh=True):
    """One ingress call of a fuzz scenario whose endpoints trace and debug, into the ring."""
    from cilium_amd.datapath import DeviceBatch
    recs, cnt, _ = dp_real.set_event_ring(8192) if fresh else dp_real.ring
    dp_real.ingress(DeviceBatch(sc.batches[0]), sc.now)
    torch.cuda.synchronize()
    return recs, cnt


def _real_scenario():
    sc = synth.fuzz(seed=7, n_packets=300, n_batches=1)
    for e in sc.lxc:
        e["flags"] |= synth.LXC_TRACE_NOTIFY | synth.LXC_DEBUG
    return sc


def test_reset_and_a_real_ring(filters):
    """The ring an ingress call leaves (drop, trace and debug records): two filters against
    monitor.match over decode_ring of the whole ring; then GF_EVD_F_RESET, after which the count
    word reads 0 and the next call's records start at slot 0."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from cilium_amd.datapath import Datapath
    sc = _real_scenario()
    dp = Datapath(sc, pin_prefix=None)
    try:
        recs, cnt = _real(dp, sc)
        n = int(cnt.item())
        assert 0 < n <= 8192
        host = recs[:n].cpu().numpy()
        dec = MON.decode_ring(host)
        assert {1, 2, 4} <= {d["type"] for d in dec}
        srcs = [d["source"] for d in dec if d["source"]]
        ep = max(set(srcs), key=srcs.count)                                  # the endpoint with most records
        for kw in (dict(types=(1, 4), frm=(ep,)), dict(related=(ep,))):
            f = MON.EventFilter(**kw)
            want = [k for k, d in enumerate(dec) if MON.match(d, **kw)]
            assert 0 < len(want) < n                                         # matches some, rejects some
            out, off, res = dp.event_drain(f)
            assert (res["count"], res["seen"], res["matched"], res["written"], res["unknown"]) == (n, n, len(want), len(want), 0)
            assert np.array_equal(out[:len(want)].cpu().numpy(), host[want])
            out, off, res = dp.event_drain(f, packed=True)
            got = MON.decode_packed(out.cpu().numpy(), off[:res["written"] + 1].cpu().numpy())
            assert got == [dec[k] for k in want]                             # a real ring's slots are zero past the wire length
            f.close()
        # the reset: the drain sees the ring, the next call starts it again
        out, off, res = dp.event_drain(filters["none"], reset=True)
        assert res["count"] == n and res["written"] == n and int(cnt.item()) == 0
        assert np.array_equal(out[:n].cpu().numpy(), host)
        recs.fill_(0xEE)
        _real(dp, sc, fresh=False)                                           # the same batch again, on the CT state it left
        n2 = int(cnt.item())
        again = recs[:n2 + 1].cpu().numpy()
        assert 0 < n2 < 8192 and set(again[:n2, 0]) <= {1, 2, 3, 4} and (again[n2] == 0xEE).all()
        out, off, res = dp.event_drain(filters["none"], first=n2)            # nothing past the count
        assert (res["count"], res["seen"], res["written"]) == (n2, 0, 0)
    finally:
        dp.close()
