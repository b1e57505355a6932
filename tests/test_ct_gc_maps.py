"""A CT GC round over many maps in one call: gf_ct_gc_maps, ctmap.GCMaps / GCRound and
Datapath.ct_gc_round (EnableConntrackGC, pkg/endpointmanager/conntrack.go:84-130: every
endpoint's local cilium_ct4_<id> / cilium_ct6_<id> and the global pair once per round).

The reference throughout is the oracle's restatement of doGC4 / doGC6 (o_ct_gc), one
call per map.  CPU: the host-shadow path, the refusals, GCRound's choice of maps.  GPU:
the multi-map sweep (k_gc_starts_multi -> k_gc_clusters_multi -> k_gc_end_multi) after
real traffic — counts, dumps, and the traffic classified after a round.
"""
import ctypes as C
import errno
import random

import numpy as np
import pytest

from cilium_amd import bpf, synth
from cilium_amd._lib import lib
from cilium_amd.maps import ctmap
from cilium_amd.synth import MapSpec, Packets
from oracle.scenario import OracleDP
import oracle.oracle as O

HASH, LRU = bpf.BPF_MAP_TYPE_HASH, bpf.BPF_MAP_TYPE_LRU_HASH
GC_MULTI = 32          # maps per chain of launches (GF_GC_MULTI, gf_kernels.hip)
CUT = 100


def _key(rng, v6, i=0):
    if v6:
        return ctmap.ct_key6(rng.randbytes(16), rng.randbytes(16), rng.getrandbits(16), rng.getrandbits(16), 6, i & 1)
    return ctmap.ct_key4(rng.getrandbits(32), rng.getrandbits(32), rng.getrandbits(16), rng.getrandbits(16), 6, i & 3)


def _filled(path, v6, lru, n, seed, max_entries=5000):
    """A pinned CT map and its oracle twin with n entries whose lifetimes straddle CUT
    (lifetime == CUT stays: the filter is lifetime < filter_time)."""
    rng = random.Random(seed)
    fd, _ = ctmap.OpenMap(bpf.MapPath(path), v6=v6, max_entries=max_entries, lru=lru)
    om = O.OMap(LRU if lru else HASH, 40 if v6 else 14, 48, max_entries)
    for i in range(n):
        k = _key(rng, v6, i)
        v = ctmap.ct_entry(rx_packets=i, lifetime=rng.choice([0, 5, CUT - 1, CUT, CUT + 1, 43300]), flags=16)
        bpf.UpdateElement(fd, k, v)
        assert om.update(k, v) == 0
    return fd, om


def _dump(fd, v6):
    m = bpf.Map("m", 0, 40 if v6 else 14, 48, 0)
    m.fd = fd
    return m.Dump()


def _raw(fds, t, want_out=True, n=None):
    """gf_ct_gc_maps itself: (return value, per-map counts)."""
    arr = (C.c_int * max(len(fds), 1))(*fds)
    out = (C.c_uint32 * max(len(fds), 1))(*([0xdead] * max(len(fds), 1)))
    rc = lib.gf_ct_gc_maps(arr, len(fds) if n is None else n, t, out if want_out else None, None)
    return rc, list(out[:len(fds)])


# ---------------------------------------------------------------- CPU: the host-shadow path
def test_gc_maps_mixed_handles_and_states():
    """IPv4 LRU, IPv6 LRU, IPv4 HASH and a never-written map in one call: per-map counts
    and dumps equal the oracle's, lifetime == filter_time stays, Flush empties them all."""
    specs = [("gcm_a", False, True, 1500), ("gcm_b", True, True, 900), ("gcm_c", False, False, 1200)]
    maps = [(_filled(p, v6, lru, n, seed=31 + j), v6) for j, (p, v6, lru, n) in enumerate(specs)]
    never, _ = ctmap.OpenMap(bpf.MapPath("gcm_never"), v6=True, max_entries=64000)
    fds = [fd for (fd, _), _ in maps] + [never]
    want = [om.ct_gc(CUT) for (_, om), _ in maps] + [0]
    assert all(w > 0 for w in want[:3])
    assert ctmap.GCMaps(fds, CUT) == want
    for (fd, om), v6 in maps:
        left = _dump(fd, v6)
        assert left == om.dump()
        lts = [ctmap.CtEntry(v).lifetime for v in left.values()]
        assert min(lts) == CUT, "lifetime == filter_time is kept, everything below is gone"
        assert bpf.GetMapInfo(fd).Entries == len(left)
    assert _dump(never, True) == {}
    # Flush: one call over the same maps in another order
    rc, cnt = _raw(fds[::-1], ctmap.MaxTime)
    assert cnt == [0] + [len(om.dump()) for (_, om), _ in maps][::-1] and rc == sum(cnt)
    assert all(_dump(fd, v6) == {} for (fd, _), v6 in maps)
    for fd in fds:
        bpf.ObjClose(fd)


def test_gc_maps_refusals_touch_nothing():
    """Every refusal comes before any map is touched: a good map first in the array
    keeps all its entries (Flush would have emptied it)."""
    (good, om), (good6, om6) = _filled("gcr_good", False, True, 300, 5), _filled("gcr_good6", True, False, 200, 6)
    before, before6 = _dump(good, False), _dump(good6, True)
    proxy = bpf.CreateMap(HASH, 10, 16, 8192)
    lpm = bpf.CreateMap(bpf.BPF_MAP_TYPE_LPM_TRIE, 8, 1, 64, bpf.BPF_F_NO_PREALLOC)
    closed = bpf.CreateMap(LRU, 14, 48, 1000)
    bpf.ObjClose(closed)
    again = bpf.ObjGet(bpf.MapPath("gcr_good"))                 # a second handle of the same map object
    assert again != good
    T = ctmap.MaxTime
    for fds, err in [([good, good6, proxy], errno.EINVAL), ([good, lpm, good6], errno.EINVAL),
                     ([good, good6, closed], errno.EBADF), ([good, good6, good], errno.EINVAL),
                     ([good, good6, again], errno.EINVAL)]:
        rc, cnt = _raw(fds, T)
        assert rc == -err, (fds, rc)
        assert cnt == [0xdead] * len(fds), "no count is written by a refused call"
        assert _dump(good, False) == before and _dump(good6, True) == before6
        with pytest.raises(bpf.BPFError) as ei:
            ctmap.GCMaps(fds, T)
        assert ei.value.errno == err
    assert lib.gf_ct_gc_maps(None, 1, T, None, None) == -errno.EFAULT
    assert lib.gf_ct_gc_maps(None, 0, T, None, None) == 0
    assert _raw([good], T, n=0) == (0, [0xdead])
    assert _raw([good] * 2, T, n=65537)[0] == -errno.E2BIG
    assert _dump(good, False) == before and _dump(good6, True) == before6
    assert ctmap.GCMaps([], T) == []
    # deleted == NULL is accepted: the return value is the sum
    w4, w6 = om.ct_gc(CUT), om6.ct_gc(CUT)
    assert _raw([good6, good], CUT, want_out=False)[0] == w4 + w6 > 0
    assert _dump(good, False) == om.dump() and _dump(good6, True) == om6.dump()
    for fd in (good, good6, proxy, lpm, again):
        bpf.ObjClose(fd)


def test_gc_round_global_pair_once():
    """GCRound over [(1, local), (2, global), (3, global), (4, local)]: the maps are
    MapNames', the global pair appears once (seenGlobal), ipv6=False leaves the v6 maps
    alone; the default opener takes the pinned maps."""
    eps = [(1, True), (2, False), (3, False), (4, True)]
    names = []
    for ep, local in [(1, True), (2, False), (4, True)]:
        n6, n4, _ = ctmap.MapNames(ep, local=local)
        names += [n6, n4]
    assert names == ["cilium_ct6_1", "cilium_ct4_1", "cilium_ct6_global", "cilium_ct4_global", "cilium_ct6_4",
                     "cilium_ct4_4"]
    maps = {n: _filled(n, "ct6" in n, True, 200 + 10 * j, seed=50 + j) for j, n in enumerate(names)}
    opened = []

    def open_map(name, v6, max_entries):
        assert ("ct6" in name) == v6
        assert max_entries == (ctmap.MapNumEntriesGlobal if name.endswith("global") else ctmap.MapNumEntriesLocal)
        opened.append(name)
        return maps[name][0]

    v4 = [n for n in names if "ct4" in n]
    want4 = {n: maps[n][1].ct_gc(CUT) for n in v4}
    assert ctmap.GCRound(eps, CUT, ipv6=False, open_map=open_map) == want4
    assert opened == v4, "each map once, the global one for endpoint 2 only"
    for n in names:
        assert _dump(maps[n][0], "ct6" in n) == maps[n][1].dump(), n      # the v6 maps still hold everything
    want = {n: (0 if "ct4" in n else maps[n][1].ct_gc(CUT)) for n in names}
    assert all(want[n] > 0 for n in names if "ct6" in n)
    got = ctmap.GCRound(eps, CUT)                               # the pinned maps, opened and closed by the round
    assert got == want and list(got) == names
    for n in names:
        assert _dump(maps[n][0], "ct6" in n) == maps[n][1].dump(), n
        bpf.ObjClose(maps[n][0])
        lib.gf_obj_unpin(bpf.MapPath(n).encode())


# ---------------------------------------------------------------- GPU: the multi-map sweep
torch = pytest.importorskip("torch")


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(0)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ct_names(sc):
    names = []
    for e in sc.lxc:
        for fam in ("ct4", "ct6"):
            if e.get(fam) and e[fam] not in names:
                names.append(e[fam])
    return names


def _ingress(dp, ref, pk, now, what):
    from cilium_amd.datapath import DeviceBatch, ING_OUT, to_numpy
    io = dp.ingress(DeviceBatch(pk), now)
    torch.cuda.synchronize()
    got, want = to_numpy(io, ING_OUT), ref.ingress(pk, now)
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, f"{what}: {len(bad)} records differ, first {bad[:1]}"
    return want


def _round(dp, ref, names, t):
    """One ct_gc_round against the oracle's per-map GC: counts, then every dump."""
    want = {n: ref.ct_gc(n, t) for n in names}
    got = dp.ct_gc_round(t)
    print("round", t, "deleted", want)
    assert got == want and list(got) == names
    for n in names:
        assert dp.dump_map(n) == ref.dump(n), n
        assert bpf.GetMapInfo(dp.fd[n]).Entries == len(ref.dump(n)), n
    return want


@pytest.mark.gpu
def test_gpu_gc_round_after_traffic():
    """Local and global maps, IPv4 and IPv6, after three batches: a round at now + 11
    (the closing entries) and one at now + 301 (the SYN-only ones), each followed by a
    batch whose records and maps still equal the oracle's — the lookups and inserts of
    that batch walk the clusters the sweep compacted and start from its counts."""
    _gpu()
    from cilium_amd.datapath import Datapath
    sc = synth.fuzz(seed=5, n_packets=20000, n_batches=3)
    made = synth.conntrack_local(sc, every=2)
    names = _ct_names(sc)
    assert set(names) == set(made) | {"ct4", "ct6"}
    dp, ref = Datapath(sc, pin_prefix=None), OracleDP(sc)
    for bi, pk in enumerate(sc.batches):
        _ingress(dp, ref, pk, sc.now + bi, f"batch {bi}")
    first = _round(dp, ref, names, sc.now + 11)
    assert sum(1 for v in first.values() if v > 0) >= 2, first
    assert any(first[n] > 0 for n in made) and any(first[n] > 0 for n in ("ct4", "ct6")), first
    _ingress(dp, ref, sc.batches[0], sc.now + 200, "after round 1")
    for n in names:
        assert dp.dump_map(n) == ref.dump(n), n
    second = _round(dp, ref, names, sc.now + 301)
    assert sum(second.values()) > 0, second
    _ingress(dp, ref, sc.batches[1], sc.now + 400, "after round 2")
    for n in names:
        assert dp.dump_map(n) == ref.dump(n), n
    dp.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n_ep", [40, 2 * GC_MULTI])
def test_gpu_gc_round_more_maps_than_one_launch(n_ep):
    """More per-endpoint maps than one chain of launches takes (40 = 32 + 8) and an exact
    multiple of it (64): two calls, one round, one more call."""
    _gpu()
    from cilium_amd.datapath import Datapath
    sc = synth.config2(n_flows=120_000, n_pairs=12_000, n_ep=n_ep, n_ids=512, n_l3=200, n_l4=400, n_wc=8,
                       n_cidr=32, ct_max=400_000)
    made = synth.conntrack_local(sc, max_entries=6000)
    assert len(made) == n_ep and n_ep > GC_MULTI
    names = _ct_names(sc)
    assert names == made
    dp, ref = Datapath(sc, pin_prefix=None), OracleDP(sc)
    pk = sc.batches[0]
    q = (pk.n + 2) // 3
    parts = [pk.slice(k * q, min(pk.n, (k + 1) * q)) for k in range(3)]
    for k in range(2):
        _ingress(dp, ref, parts[k], sc.now + k, f"call {k}")
    got = _round(dp, ref, names, sc.now + 302)                  # the SYN-only entries of both calls
    assert sum(1 for v in got.values() if v > 0) > GC_MULTI, "maps of the second chain deleted too"
    _ingress(dp, ref, parts[2], sc.now + 303, "call after the round")
    for n in names:
        assert dp.dump_map(n) == ref.dump(n), n
    dp.close()


def _full_slot(fd, s, ksz):
    """Slot s of a map on its host shadow holds an entry (the dump cursor is a slot index:
    a chunk of no entries returns the first FULL slot at or after the cursor)."""
    _, _, nxt, _ = bpf.LookupBatch(fd, s, 0, ksz, 48)
    return nxt == s


def _wrapping_keys(v6, max_entries, seed):
    """Keys whose home is the last 128-B line of a 64-slot table (the library's own hash,
    found through the host shadow of scratch maps), enough of them that their cluster
    runs from that line over slot 63 into slots 0 and 1."""
    rng = random.Random(seed)
    ksz, spl = (40, 2) if v6 else (14, 4)
    keys = []
    while len(keys) < spl + 2:
        k = _key(rng, v6)
        fd = bpf.CreateMap(HASH, ksz, 48, max_entries)
        bpf.UpdateElement(fd, k, ctmap.ct_entry())
        home = bpf.LookupBatch(fd, 0, 0, ksz, 48)[2]
        bpf.ObjClose(fd)
        if home == 64 - spl:
            keys.append(k)
    return keys, rng


@pytest.mark.gpu
def test_gpu_gc_smallest_tables_side_by_side():
    """Three 64-slot maps (two bit words each) of each family next to each other in one
    call: the first holds a probe cluster that wraps from slot 63 to slot 0 and loses
    entries in front of the wrap (the survivors move back across it), the middle one is
    empty, every entry of the last is below the cutoff.  Counts, dumps and lookups of
    every survivor through the probe sequence equal the oracle's; no map's walk reaches
    its neighbour."""
    _gpu()
    from cilium_amd.datapath import Datapath
    sc = synth.fuzz(seed=3, n_packets=4000, n_batches=1)
    tiny, trio = [], {}
    for v6 in (False, True):
        fam, ksz, mx = ("ct6", 40, 16) if v6 else ("ct4", 14, 8)
        wrap, rng = _wrapping_keys(v6, mx, seed=77 + v6)
        others = [_key(rng, v6) for _ in range(2)]
        lts = [CUT - 1, CUT + 5, 0] + [CUT + 7] * (len(wrap) - 3) + [CUT - 1, CUT]
        a = (wrap + others, lts)
        c = ([_key(rng, v6) for _ in range(mx)], [rng.choice([0, 7, CUT - 1]) for _ in range(mx)])
        for j, (keys, lifetimes) in enumerate([a, ([], []), c]):
            e = sc.lxc[j]
            name = f"{fam}_{e['lxc_id']}"
            k = np.frombuffer(b"".join(keys), np.uint8).reshape(-1, ksz)
            v = np.frombuffer(b"".join(ctmap.ct_entry(rx_packets=i, lifetime=lt, flags=16)
                                       for i, lt in enumerate(lifetimes)), np.uint8).reshape(-1, 48)
            sc.add_map(MapSpec(name, HASH, ksz, 48, mx, 0, k.copy(), v.copy()))
            e[fam] = name
            trio.setdefault(fam, []).append(name)
            tiny.append(e["lxc_id"])
    dp, ref = Datapath(sc, pin_prefix=None), OracleDP(sc)
    for fam, ksz in (("ct4", 14), ("ct6", 40)):
        fd = dp.fd[trio[fam][0]]
        assert _full_slot(fd, 63, ksz) and _full_slot(fd, 0, ksz) and _full_slot(fd, 1, ksz), "the cluster wraps"
        assert not _full_slot(fd, 64 - 128 // (32 if ksz == 14 else 64) - 1, ksz), "and starts at the last line"
    # the other endpoints' traffic: the classify call pushes every bound map and leaves it device-owned
    pk = sc.batches[0]
    m = ~np.isin(pk.lxc_id, tiny)
    f = lambda x: None if x is None else x[m]
    part = Packets(pk.frames[m], pk.lens[m], f(pk.src_identity), f(pk.ifindex), f(pk.lxc_id), f(pk.tc_index),
                   f(pk.flow_hash))
    _ingress(dp, ref, part, sc.now, "traffic")
    order = trio["ct4"] + trio["ct6"]
    want = [ref.ct_gc(n, CUT) for n in order]
    assert want[1] == want[4] == 0 and want[2] == 8 and want[5] == 16 and want[0] == want[3] == 3
    assert ctmap.GCMaps([dp.fd[n] for n in order], CUT, _stream()) == want
    for n in order:
        left = ref.dump(n)
        assert dp.dump_map(n) == left, n
        assert bpf.GetMapInfo(dp.fd[n]).Entries == len(left), n
        for k, v in left.items():                               # walks home -> key: no EMPTY slot in between
            assert bpf.LookupElement(dp.fd[n], k, 48) == v, n
    for n in ("ct4", "ct6"):
        assert dp.dump_map(n) == ref.dump(n), n
    dp.close()


@pytest.mark.gpu
def test_gpu_gc_mixed_state_in_one_call():
    """A map still on its host shadow, a device-owned map traffic has written and a map
    that never materialised in one array: the counts come back in array order."""
    _gpu()
    from cilium_amd.datapath import Datapath
    sc = synth.fuzz(seed=5, n_packets=20000, n_batches=2)
    dp, ref = Datapath(sc, pin_prefix=None), OracleDP(sc)
    for bi, pk in enumerate(sc.batches):
        _ingress(dp, ref, pk, sc.now + bi, f"batch {bi}")
    host, om = _filled("gcx_host", True, False, 700, seed=9)
    never = bpf.CreateMap(LRU, 14, 48, 64000)
    t = sc.now + 11
    # lifetimes of the host map straddle CUT, not t: use one cutoff that bites in both
    want_dev4, want_dev6, want_host = ref.ct_gc("ct4", t), ref.ct_gc("ct6", t), om.ct_gc(t)
    assert want_dev4 > 0 and want_host > 0
    got = ctmap.GCMaps([host, dp.fd["ct4"], never, dp.fd["ct6"]], t, _stream())
    assert got == [want_host, want_dev4, 0, want_dev6]
    assert _dump(host, True) == om.dump()
    assert dp.dump_map("ct4") == ref.dump("ct4") and dp.dump_map("ct6") == ref.dump("ct6")
    assert bpf.GetMapInfo(never).Entries == 0
    bpf.ObjClose(host)
    bpf.ObjClose(never)
    lib.gf_obj_unpin(bpf.MapPath("gcx_host").encode())
    dp.close()


@pytest.mark.gpu
def test_gpu_gc_round_reopens_full_hash_maps():
    """Per-endpoint HASH CT maps filled to max_entries with unrelated entries: every new
    connection is DROP_CT_CREATE_FAILED; after a round that deletes those entries the
    device counts are exact again and the next call inserts, as in the oracle."""
    _gpu()
    from cilium_amd.datapath import Datapath
    sc = synth.fuzz(seed=4, n_packets=20000, n_batches=2)
    made = [n for n in synth.conntrack_local(sc, every=2) if n.startswith("ct4_")]
    rng, mx = random.Random(12), 4000
    for n in made:
        k = np.frombuffer(b"".join(_key(rng, False) for _ in range(mx)), np.uint8).reshape(-1, 14)
        v = np.frombuffer(ctmap.ct_entry(lifetime=sc.now + 50, flags=16) * mx, np.uint8).reshape(-1, 48)
        sc.maps[n] = MapSpec(n, HASH, 14, 48, mx, 0, k.copy(), v.copy())
    names = _ct_names(sc)
    dp, ref = Datapath(sc, pin_prefix=None), OracleDP(sc)
    r0 = _ingress(dp, ref, sc.batches[0], sc.now, "full maps")
    assert (r0["reason"] == 155).sum() > 0, "DROP_CT_CREATE_FAILED while the maps are full"
    assert all(len(ref.dump(n)) == mx for n in made)
    got = _round(dp, ref, names, sc.now + 51)
    assert all(got[n] == mx for n in made), got
    r1 = _ingress(dp, ref, sc.batches[1], sc.now + 52, "after the round")
    assert (r1["reason"] == 155).sum() == 0
    assert sum(len(ref.dump(n)) for n in made) > 0, "the maps take inserts again"
    for n in names:
        assert dp.dump_map(n) == ref.dump(n), n
        assert bpf.GetMapInfo(dp.fd[n]).Entries == len(ref.dump(n)), n
    dp.close()


@pytest.mark.gpu
def test_gpu_gc_maps_equals_one_map_calls():
    """The same scenario twice, one collected by a loop of gf_ct_gc and one by a single
    gf_ct_gc_maps: identical counts, dumps and gf_map_get_info element counts."""
    _gpu()
    from cilium_amd.datapath import Datapath, DeviceBatch
    sc = synth.fuzz(seed=6, n_packets=20000, n_batches=3)
    synth.conntrack_local(sc, every=2, max_entries=900)         # small: evictions leave FREE slots to clear
    names = _ct_names(sc)
    dps = [Datapath(sc, pin_prefix=None), Datapath(sc, pin_prefix=None)]
    for dp in dps:
        for bi, pk in enumerate(sc.batches):
            dp.ingress(DeviceBatch(pk), sc.now + bi)
    torch.cuda.synchronize()
    for t in (sc.now + 11, sc.now + 301):
        one = [lib.gf_ct_gc(dps[0].fd[n], t, _stream()) for n in names]
        many = ctmap.GCMaps([dps[1].fd[n] for n in names], t, _stream())
        assert one == many and min(one) >= 0, (t, one, many)
        assert sum(one) > 0
        for n in names:
            assert dps[0].dump_map(n) == dps[1].dump_map(n), n
            assert bpf.GetMapInfo(dps[0].fd[n]).Entries == bpf.GetMapInfo(dps[1].fd[n]).Entries, n
    for dp in dps:
        dp.close()
