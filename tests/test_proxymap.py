"""cilium_proxy4 / cilium_proxy6 GC, Flush and redirect-close cleanup: gf_proxy_gc,
gf_proxy_cleanup_port and the pkg/maps/proxymap mirror (cilium_amd.maps.proxymap).

CPU part: byte layouts and the host-shadow path of both calls.  GPU part: the device
sweep (k_gc_starts -> k_px_gc) on small device-owned tables built so that probe clusters
wrap the end of the slot array and cross a 32-slot word of the cluster-start bitmap, after
real traffic against tests/ctoff_model.py, the count / bound reset, and stream ordering.
"""
import ctypes as C
import errno
import struct

import numpy as np
import pytest

from cilium_amd import bpf, synth
from cilium_amd._lib import lib, gf_map_info, gf_prof_rec
from cilium_amd.maps import proxymap
from cilium_amd.synth import Packets
from oracle.scenario import OracleDP
from tests import ctoff_model as M

V4, V6 = (10, 16), (22, 28)                             # (key, value) sizes
LT_OFF = {10: 12, 22: 24}                               # value offset of lifetime
DPORT_OFF = {10: 4, 22: 16}                             # key offsets of dport / nexthdr
NH_OFF = {10: 8, 22: 20}


def _dump(fd, ksz, vsz):
    """The reference's loop: GetNextKey + LookupElement, in the walk's order."""
    out, key = [], None
    while True:
        try:
            key = bpf.GetNextKey(fd, key, ksz)
        except bpf.BPFError as e:
            assert e.errno == errno.ENOENT
            return out
        out.append((key, bpf.LookupElement(fd, key, vsz)))


def _count(fd):
    info = gf_map_info()
    assert lib.gf_map_get_info(fd, C.byref(info)) == 0
    return info.n_entries


def _rand_entries(rng, ksz, vsz, n, dports=None, nexthdrs=(6, 17)):
    """n distinct proxy keys (pad byte 0) and values; lifetimes are filled in by the caller."""
    alen = ksz - 6
    keys = set()
    while len(keys) < n:
        dport = int(rng.choice(dports)) if dports is not None else int(rng.integers(0, 65536))
        keys.add(bytes(rng.integers(0, 256, alen, dtype=np.uint8)) +
                 struct.pack("<HHBB", dport, int(rng.integers(0, 65536)), int(rng.choice(nexthdrs)), 0))
    keys = sorted(keys)
    rng.shuffle(keys)
    vals = [bytes(rng.integers(0, 256, vsz - 4, dtype=np.uint8)) for _ in keys]
    return keys, vals


# ---------------------------------------------------------------- layouts
def test_layouts_pack_to_the_reference_bytes():
    k4 = proxymap.Proxy4Key(bytes([10, 1, 0, 2]), DPort=0x2328, SPort=0xC001, Nexthdr=6)
    assert k4.pack() == bytes([10, 1, 0, 2, 0x28, 0x23, 0x01, 0xC0, 6, 0]) and len(k4.pack()) == 10
    assert k4.ToNetwork().pack() == bytes([10, 1, 0, 2, 0x23, 0x28, 0xC0, 0x01, 6, 0])
    v4 = proxymap.Proxy4Value(bytes([10, 2, 0, 9]), OrigDPort=80, SourceIdentity=0x01020304, Lifetime=5720)
    assert v4.pack() == bytes([10, 2, 0, 9, 80, 0, 0, 0, 4, 3, 2, 1, 0x58, 0x16, 0, 0]) and len(v4.pack()) == 16
    assert v4.ToNetwork().pack() == bytes([10, 2, 0, 9, 0, 80, 0, 0, 4, 3, 2, 1, 0x58, 0x16, 0, 0])
    a6 = bytes([0xf0, 0x0d]) + bytes(13) + bytes([1])
    k6 = proxymap.Proxy6Key(a6, DPort=9000, SPort=1, Nexthdr=17)
    assert k6.pack() == a6 + bytes([0x28, 0x23, 1, 0, 17, 0]) and len(k6.pack()) == 22
    v6 = proxymap.Proxy6Value(a6, OrigDPort=0x1F90, SourceIdentity=258, Lifetime=0xFFFFFFFE)
    assert v6.pack() == a6 + bytes([0x90, 0x1F, 0, 0, 2, 1, 0, 0, 0xFE, 0xFF, 0xFF, 0xFF]) and len(v6.pack()) == 28
    for x in (k4, v4, k6, v6):                          # ToNetwork is an involution that keeps the type
        assert x.ToNetwork().ToNetwork() == x and type(x.ToNetwork()) is type(x)
        assert type(x).unpack(x.pack()) == x
    # String(): "%s (%d) => %d" over HostPort() = JoinHostPort(SAddr, SPort); "%s:%d identity %d lifetime %d"
    assert k4.String() == "10.1.0.2:49153 (6) => 9000"
    assert v4.String() == "10.2.0.9:80 identity 16909060 lifetime 5720"
    assert k6.String() == "[f00d::1]:1 (17) => 9000"
    assert v6.String() == "f00d::1:8080 identity 258 lifetime 4294967294" and v6.HostPort() == "[f00d::1]:8080"
    assert proxymap.MaxEntries == 524288


def test_flush_filter_time_is_the_reference_quirk():
    """gc(math.MaxUint64): uint32(18446744073709551615 / 10^9) = 1266874889, not 0xFFFFFFFF."""
    assert proxymap.FlushFilterTime == 1266874889 == (18446744073709551615 // 10 ** 9) % 2 ** 32
    assert proxymap.filter_time(5000 * 10 ** 9 + 999999999) == 5000          # truncated
    assert proxymap.filter_time((2 ** 32 + 7) * 10 ** 9) == 7                # uint32(tsec)


# ---------------------------------------------------------------- host shadow
@pytest.mark.parametrize("ksz,vsz", [V4, V6])
def test_gc_on_the_host_shadow(ksz, vsz):
    rng = np.random.default_rng(ksz)
    fd = bpf.CreateMap(bpf.BPF_MAP_TYPE_HASH, ksz, vsz, 4096)
    assert lib.gf_proxy_gc(fd, 5000, None) == 0         # nothing inserted yet
    t, n = 70000, 1000
    keys, vals = _rand_entries(rng, ksz, vsz, n)
    lts = rng.integers(t - 50, t + 50, n).astype(np.uint32)
    lts[::97] = t                                       # several exactly at the cutoff: they stay
    lts[1], lts[2], lts[3] = 0, 0xFFFFFFFE, t - 1
    assert (lts == t).sum() >= 10
    ents = {k: v + struct.pack("<I", int(lt)) for k, v, lt in zip(keys, vals, lts)}
    for k, v in ents.items():
        bpf.UpdateElement(fd, k, v)
    assert lib.gf_proxy_gc(fd, t, None) == int((lts < t).sum()) > 100
    want = {k: v for k, v in ents.items() if struct.unpack_from("<I", v, LT_OFF[ksz])[0] >= t}
    got = _dump(fd, ksz, vsz)
    assert len(got) == len(want) and dict(got) == want and _count(fd) == len(want)
    assert lib.gf_proxy_gc(fd, t, None) == 0
    # Flush (the module's filter time): everything below 1266874889 goes, 0xFFFFFFFE stays; the C call takes any u32
    fd4, fd6 = (fd, None) if ksz == 10 else (None, fd)
    assert proxymap.Flush(fd4, fd6) == len(want) - 1
    assert [struct.unpack_from("<I", v, LT_OFF[ksz])[0] for _, v in _dump(fd, ksz, vsz)] == [0xFFFFFFFE]
    assert lib.gf_proxy_gc(fd, 0xFFFFFFFF, None) == 1 and _dump(fd, ksz, vsz) == [] and _count(fd) == 0
    # GC(fd4, fd6, mtime_ns): tsec = time / 1e9 truncated
    bpf.UpdateElement(fd, keys[0], vals[0] + struct.pack("<I", 41))
    bpf.UpdateElement(fd, keys[1], vals[1] + struct.pack("<I", 42))
    assert proxymap.GC(fd4, fd6, 42 * 10 ** 9 + 999999999) == 1
    assert dict(_dump(fd, ksz, vsz)) == {keys[1]: vals[1] + struct.pack("<I", 42)}


@pytest.mark.parametrize("ksz,vsz", [V4, V6])
def test_port_cleanup_on_the_host_shadow(ksz, vsz):
    rng = np.random.default_rng(100 + ksz)
    fd = bpf.CreateMap(bpf.BPF_MAP_TYPE_HASH, ksz, vsz, 4096)
    port, other = 9001, 9002
    raw = lambda p: ((p & 0xff) << 8) | (p >> 8)
    keys, vals = _rand_entries(rng, ksz, vsz, 600, dports=[raw(port), raw(other), port], nexthdrs=(6, 17, 1))
    ents = {k: v + struct.pack("<I", 5000) for k, v in zip(keys, vals)}
    for k, v in ents.items():
        bpf.UpdateElement(fd, k, v)
    hit = lambda k: struct.unpack_from("<H", k, DPORT_OFF[ksz])[0] == raw(port) and k[NH_OFF[ksz]] == 6
    nhit = sum(hit(k) for k in ents)
    same_port_udp = sum(struct.unpack_from("<H", k, DPORT_OFF[ksz])[0] == raw(port) and k[NH_OFF[ksz]] == 17 for k in ents)
    assert nhit > 30 and same_port_udp > 30
    fd4, fd6 = (fd, None) if ksz == 10 else (None, fd)
    assert proxymap.CleanupOnRedirectClose(fd4, fd6, port) == nhit
    assert dict(_dump(fd, ksz, vsz)) == {k: v for k, v in ents.items() if not hit(k)}
    assert lib.gf_proxy_cleanup_port(fd, raw(port), None) == 0
    # Lookup converts the key to network order and the value back; Delete takes the key as given
    k = next(k for k in ents if not hit(k))
    kt, vt = (proxymap.Proxy4Key, proxymap.Proxy4Value) if ksz == 10 else (proxymap.Proxy6Key, proxymap.Proxy6Value)
    v = proxymap.Lookup(fd4, fd6, kt.unpack(k).ToNetwork())
    assert v == vt.unpack(ents[k]).ToNetwork() and v.GetSourceIdentity() == struct.unpack_from("<I", ents[k], ksz - 2)[0]
    proxymap.Delete(fd4, fd6, kt.unpack(k))
    with pytest.raises(bpf.BPFError) as ei:
        proxymap.Lookup(fd4, fd6, kt.unpack(k).ToNetwork())
    assert ei.value.errno == errno.ENOENT


def test_refusals():
    ct4 = bpf.CreateMap(bpf.BPF_MAP_TYPE_LRU_HASH, 14, 48, 1024)
    pol = bpf.CreateMap(bpf.BPF_MAP_TYPE_HASH, 8, 24, 1024)
    lpm = bpf.CreateMap(bpf.BPF_MAP_TYPE_LPM_TRIE, 8, 1, 64, bpf.BPF_F_NO_PREALLOC)
    odd = bpf.CreateMap(bpf.BPF_MAP_TYPE_HASH, 10, 28, 64)                   # a v4 key with the v6 value
    for fd in (ct4, pol, lpm, odd):
        assert lib.gf_proxy_gc(fd, 5000, None) == -errno.EINVAL
        assert lib.gf_proxy_cleanup_port(fd, 80, None) == -errno.EINVAL
    for ksz, vsz in (V4, V6):
        px = bpf.CreateMap(bpf.BPF_MAP_TYPE_HASH, ksz, vsz, 64)
        assert lib.gf_ct_gc(px, 5000, None) == -errno.EINVAL                 # gf_ct_gc keeps refusing these maps
        assert lib.gf_proxy_gc(px, 5000, None) == 0
        bpf.ObjClose(px)
        assert lib.gf_proxy_gc(px, 5000, None) == -errno.EBADF
        assert lib.gf_proxy_cleanup_port(px, 80, None) == -errno.EBADF
    assert lib.gf_proxy_gc(0, 5000, None) == -errno.EBADF


# ---------------------------------------------------------------- small tables: the key sets
def _hash(key):
    """gf_key_hash(GF_HASH_PLAIN) of gf_common.h: murmur3-style mix over the key as
    little-endian u32 words, zero-padded, seeded with the key length."""
    r = lambda x, n: ((x << n) | (x >> (32 - n))) & 0xFFFFFFFF
    h = 0x9747b28c ^ len(key)
    for w, in struct.iter_unpack("<I", key + bytes(-len(key) % 4)):
        k = r((w * 0xcc9e2d51) & 0xFFFFFFFF, 15) * 0x1b873593 & 0xFFFFFFFF
        h = (r(h ^ k, 13) * 5 + 0xe6546b64) & 0xFFFFFFFF
    h ^= h >> 16
    h = h * 0x85ebca6b & 0xFFFFFFFF
    h ^= h >> 13
    h = h * 0xc2b2ae35 & 0xFFFFFFFF
    return h ^ (h >> 16)


def _geometry(ksz, max_entries):
    """The proxy maps' slot array (gf_node_config: a power of two >= max(64, 2 x max_entries))
    and slots per 128-B line (gf_htab_layout: 32-B slots for 10/16, 64-B for 22/28)."""
    n = 64
    while n < 2 * max_entries:
        n *= 2
    return n, 4 if ksz == 10 else 2


def _home(key, nslots, spl):
    return (_hash(key) & (nslots - 1)) & ~(spl - 1)


def _layout(keys, nslots, spl):
    """Slot of each key after inserting them in order into an empty table (linear probing
    from the first slot of the home line)."""
    slot_of, used = {}, [False] * nslots
    for k in keys:
        i = _home(k, nslots, spl)
        while used[i]:
            i = (i + 1) & (nslots - 1)
        used[i] = True
        slot_of[k] = i
    return slot_of, used


SEEDS = 16


def _key_set(ksz, vsz, max_entries, seed, by_port):
    """max_entries keys for one fill.  Every 4th seed starts with 6 keys homed in the last
    line of the slot array (their cluster runs past the end into slot 0), every 4th + 1 with
    6 keys homed in the line that ends at slot 31 (their cluster crosses into the bitmap's
    second word); the rest is random.  Victims alternate with survivors in insertion order."""
    rng = np.random.default_rng([ksz, max_entries, seed, int(by_port)])
    nslots, spl = _geometry(ksz, max_entries)
    raw = lambda p: ((p & 0xff) << 8) | (p >> 8)
    dports = [raw(9001), raw(9002)] if by_port else None
    pool, vals = _rand_entries(rng, ksz, vsz, 24 * max_entries, dports=dports)
    target = {0: nslots - spl, 1: 32 - spl}.get(seed % 4)
    first = [k for k in pool if _home(k, nslots, spl) == target][:6] if target is not None else []
    assert target is None or len(first) == 6
    keys = first + [k for k in pool if k not in first][:max_entries - len(first)]
    val_of = dict(zip(pool, vals))
    t = 6000
    if by_port:
        ents = [(k, val_of[k] + struct.pack("<I", t)) for k in keys]
        victim = [struct.unpack_from("<H", k, DPORT_OFF[ksz])[0] == raw(9001) and k[NH_OFF[ksz]] == 6 for k in keys]
    else:
        lts = [t - 1 if j % 2 == 0 else (t if j % 8 == 1 else t + 1) for j in range(len(keys))]
        ents = [(k, val_of[k] + struct.pack("<I", lt)) for k, lt in zip(keys, lts)]
        victim = [lt < t for lt in lts]
    return ents, victim, t


@pytest.mark.parametrize("ksz,vsz", [V4, V6])
@pytest.mark.parametrize("max_entries", [24, 48, 96])
@pytest.mark.parametrize("by_port", [False, True])
def test_small_table_key_sets_reach_the_edge_cases(ksz, vsz, max_entries, by_port):
    """The key sets of test_gpu_small_tables, laid out on the CPU with the table's hash
    restated above: over the 16 seeds of a size, clusters that wrap the end of the slot
    array and clusters that cross a 32-slot word of the start bitmap both occur, with
    victims and survivors inside them.  (The GPU test checks this layout against the
    device table's own get_next_key order before it sweeps.)"""
    nslots, spl = _geometry(ksz, max_entries)
    wraps = crossings = 0
    for seed in range(SEEDS):
        ents, victim, _ = _key_set(ksz, vsz, max_entries, seed, by_port)
        assert len(ents) == max_entries == len({k for k, _ in ents})
        assert 0 < sum(victim) < max_entries
        slot_of, used = _layout([k for k, _ in ents], nslots, spl)
        assert not all(used)
        # an entry sitting across the edge from its home line, i.e. a cluster over the edge that a walk must follow
        over = lambda k, edge: ((slot_of[k] - _home(k, nslots, spl)) % nslots) > ((edge - 1 - _home(k, nslots, spl)) % nslots)
        wraps += any(over(k, 0) for k, _ in ents)
        crossings += any(over(k, 32) for k, _ in ents)
    assert wraps >= SEEDS // 4 and crossings >= SEEDS // 4, (wraps, crossings)


# ---------------------------------------------------------------- GPU
torch = pytest.importorskip("torch")


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(0)


def _subset(pk, m):
    f = lambda x: None if x is None else x[m]
    return Packets(pk.frames[m], pk.lens[m], f(pk.src_identity), f(pk.ifindex), f(pk.lxc_id), f(pk.tc_index),
                   f(pk.flow_hash))


def proxy_scenario(max4=65536, max6=65536, n_packets=4000):
    """The all-CT-off scenario of test_conntrack_off.test_gpu_proxy_redirects_all_off:
    every endpoint has {id, 0, proto} policy entries with a proxy port."""
    sc = synth.fuzz(seed=6, n_packets=n_packets, n_batches=2)
    sc.add_map(synth.MapSpec("cilium_proxy4", synth.HASH, 10, 16, max4, 0))
    sc.add_map(synth.MapSpec("cilium_proxy6", synth.HASH, 22, 28, max6, 0))
    sc.node = {"proxy4": "cilium_proxy4", "proxy6": "cilium_proxy6", "ipv4_gateway": 0xfffff50a,
               "host_ip6": bytes(range(16))}
    off = synth.conntrack_off(sc)
    for j, e in enumerate(sc.lxc):
        m = sc.maps[e["policy"]]
        ids = np.array([1, 2, 256, 257, 258, 259], np.uint32)
        k = synth.policy_keys(ids, np.zeros(6), np.array([6, 17, 6, 17, 1, 58]))
        v = synth.policy_vals(np.array([9000 + j, 0, 9100 + j, 9200, 9300, 9400]))
        m.keys, m.vals = synth.dedup(np.concatenate([k, m.keys]), np.concatenate([v, m.vals]))
    return sc, off


class Run:
    """A datapath beside the model and the oracle: classify a batch and compare."""

    def __init__(self, sc, off):
        from cilium_amd.datapath import Datapath
        self.sc, self.off = sc, off
        self.dp, self.ref, self.model = Datapath(sc, pin_prefix=None), OracleDP(sc), M.CtOffModel(sc)

    def expect(self, pk, now):
        idx, mrec, _ = self.model.batch(pk, self.ref.parse(pk), now)
        offm = np.zeros(pk.n, bool)
        offm[idx] = True
        assert np.array_equal(offm, np.isin(pk.lxc_id, self.off))
        want = np.zeros(pk.n, M.ING_OUT)
        want[idx] = mrec
        want[~offm] = self.ref.ingress(_subset(pk, ~offm), now)
        return want

    def classify(self, pk, now):
        from cilium_amd.datapath import DeviceBatch, ING_OUT, to_numpy
        io = self.dp.ingress(DeviceBatch(pk), now)
        torch.cuda.synchronize()
        return to_numpy(io, ING_OUT)

    def step(self, pk, now):
        got, want = self.classify(pk, now), self.expect(pk, now)
        bad = np.nonzero(got != want)[0]
        assert len(bad) == 0, f"{len(bad)} records differ, first packet {bad[:1]}: {got[bad[:1]]} != {want[bad[:1]]}"
        return got

    def maps_equal_model(self):
        assert self.dp.dump_map("cilium_proxy4") == self.model.proxy4
        assert self.dp.dump_map("cilium_proxy6") == self.model.proxy6


def _kernel_launches(name):
    recs = (gf_prof_rec * 64)()
    n = lib.gf_prof_read(recs, 64)
    return sum(r.count for r in recs[:n] if r.name.decode() == name)


@pytest.mark.gpu
@pytest.mark.parametrize("max_entries", [24, 48, 96])
@pytest.mark.parametrize("by_port", [False, True])
def test_gpu_small_tables(max_entries, by_port):
    """Device-owned proxy maps of 64 / 128 / 256 slots, filled to max_entries through the
    map API, swept by lifetime or by port, 16 key sets per size and family (the sets of
    test_small_table_key_sets_reach_the_edge_cases: wrapping and word-crossing clusters).
    Before each sweep the device table's get_next_key order must equal the CPU layout of
    the key set, which is what establishes that those clusters are really there.  After it:
    every survivor is found with its value, every victim is ENOENT, the walk yields exactly
    the survivors and the count agrees; then the victims go back in (probing through the
    compacted clusters) and everything is found again."""
    _gpu()
    sc, off = proxy_scenario(max_entries, max_entries, n_packets=400)
    run = Run(sc, off)
    dp = run.dp
    # one redirect makes both maps device-owned (the proxy log's apply marks them)
    pk = sc.batches[0]
    want = run.expect(pk, sc.now)
    i = int(np.nonzero(want["flags"] & M.ING_F_PROXY)[0][0])
    run.model.proxy4.clear(), run.model.proxy6.clear()
    one = _subset(pk, np.array([i]))
    got = run.step(one, sc.now)
    assert got["flags"][0] & M.ING_F_PROXY and len(run.model.proxy4) + len(run.model.proxy6) == 1
    run.maps_equal_model()
    lib.gf_prof_enable(1)
    try:
        assert dp.proxy_gc("cilium_proxy4", 0xFFFFFFFF) + dp.proxy_gc("cilium_proxy6", 0xFFFFFFFF) == 1
        assert _kernel_launches("k_px_gc") == 2         # both on the device, the host shadow is not authoritative
    finally:
        lib.gf_prof_enable(0)
    for name, (ksz, vsz) in (("cilium_proxy4", V4), ("cilium_proxy6", V6)):
        fd = dp.fd[name]
        nslots, spl = _geometry(ksz, max_entries)
        for seed in range(SEEDS):
            ents, victim, t = _key_set(ksz, vsz, max_entries, seed, by_port)
            for k, v in ents:
                bpf.UpdateElement(fd, k, v)
            assert _count(fd) == max_entries
            with pytest.raises(bpf.BPFError) as ei:     # full: a new key is refused, as in the kernel
                bpf.UpdateElement(fd, bytes(ksz), bytes(vsz))
            assert ei.value.errno == errno.E2BIG
            slot_of, _ = _layout([k for k, _ in ents], nslots, spl)
            walk = _dump(fd, ksz, vsz)
            assert [k for k, _ in walk] == sorted(slot_of, key=slot_of.get), (name, seed)
            nv = sum(victim)
            if by_port:
                assert dp.proxy_cleanup_port(name, 9001) == nv, (name, seed)
            else:
                assert dp.proxy_gc(name, t) == nv, (name, seed)
            live = {k: v for (k, v), dead in zip(ents, victim) if not dead}

            def check(present, absent):
                for k, v in present.items():
                    assert bpf.LookupElement(fd, k, vsz) == v, (name, seed)
                for k in absent:
                    with pytest.raises(bpf.BPFError) as ei:
                        bpf.LookupElement(fd, k, vsz)
                    assert ei.value.errno == errno.ENOENT, (name, seed)
                walk = _dump(fd, ksz, vsz)
                assert len(walk) == len(present) and dict(walk) == present, (name, seed)
                assert _count(fd) == len(present), (name, seed)

            check(live, [k for (k, _), dead in zip(ents, victim) if dead])
            for (k, v), dead in zip(ents, victim):
                if dead:
                    bpf.UpdateElement(fd, k, v)
            check(dict(ents), [])
            assert dp.proxy_gc(name, 0xFFFFFFFF) == max_entries     # empty again for the next key set
            assert _count(fd) == 0 and _dump(fd, ksz, vsz) == []
    dp.close()


@pytest.mark.gpu
def test_gpu_gc_after_real_traffic():
    """Two batches of redirect-heavy traffic (batch 0 at now, batch 1 at now + 1), then
    gf_proxy_gc(now + 720 + 1) on both maps: exactly the keys last written by batch 0 go
    (lifetime now + 720 < cutoff <= now + 721).  Batch 0 again at now + 2 continues from
    the swept maps: no duplicate keys, nothing lost."""
    _gpu()
    sc, off = proxy_scenario()
    run = Run(sc, off)
    run.step(sc.batches[0], sc.now)
    run.step(sc.batches[1], sc.now + 1)
    run.maps_equal_model()
    cut = sc.now + 720 + 1
    for name, d, lt_off in (("cilium_proxy4", run.model.proxy4, 12), ("cilium_proxy6", run.model.proxy6, 24)):
        old = [k for k, v in d.items() if struct.unpack_from("<I", v, lt_off)[0] == sc.now + 720]
        assert 0 < len(old) < len(d), name
        assert run.dp.proxy_gc(name, cut) == len(old), name
        for k in old:
            del d[k]
        assert run.dp.proxy_gc(name, cut) == 0, name
    run.maps_equal_model()
    assert _count(run.dp.fd["cilium_proxy4"]) == len(run.model.proxy4)
    run.step(sc.batches[0], sc.now + 2)
    run.maps_equal_model()
    assert _count(run.dp.fd["cilium_proxy4"]) == len(run.model.proxy4)
    assert _count(run.dp.fd["cilium_proxy6"]) == len(run.model.proxy6)
    # the redirect of one proxy port closes: its TCP entries go, on both maps
    port = next(struct.unpack_from(">H", k, 4)[0] for k in run.model.proxy4 if k[8] == 6)
    n = 0
    for name, d, ksz in (("cilium_proxy4", run.model.proxy4, 10), ("cilium_proxy6", run.model.proxy6, 22)):
        hit = [k for k in d if struct.unpack_from(">H", k, DPORT_OFF[ksz])[0] == port and k[NH_OFF[ksz]] == 6]
        for k in hit:
            del d[k]
        n += len(hit)
    assert n > 0
    assert proxymap.CleanupOnRedirectClose(run.dp.fd["cilium_proxy4"], run.dp.fd["cilium_proxy6"], port) == n
    run.maps_equal_model()
    run.dp.close()


@pytest.mark.gpu
def test_gpu_flush_brings_the_bound_back_down():
    """cilium_proxy4 sized M so that batch 0's distinct keys fit, batch 1's fit, and their
    union does not.  Without a flush batch 1 runs into the full map (DROP_PROXYMAP_CREATE_FAILED,
    161).  With Flush between the batches it does not: the device count and the host's
    bound of it were reset with the table."""
    _gpu()
    probe, off = proxy_scenario()
    ref, keys = OracleDP(probe), []
    for bi, pk in enumerate(probe.batches):
        model = M.CtOffModel(probe)
        model.batch(pk, ref.parse(pk), probe.now + bi)
        keys.append(set(model.proxy4))
    m = max(len(keys[0]), len(keys[1]))
    assert len(keys[0]) <= m and len(keys[1]) <= m and len(keys[0] | keys[1]) > m

    sc, off = proxy_scenario(max4=m)
    a = Run(sc, off)
    a.step(sc.batches[0], sc.now)
    got, want = a.classify(sc.batches[1], sc.now + 1), a.expect(sc.batches[1], sc.now + 1)
    full = got["reason"] == 161
    assert full.any() and (got["action"][full] == 2).all() and (want["flags"][full] & M.ING_F_PROXY).all()
    assert np.array_equal(got[~full], want[~full])
    assert _count(a.dp.fd["cilium_proxy4"]) == m
    a.dp.close()

    sc, off = proxy_scenario(max4=m)
    b = Run(sc, off)
    b.step(sc.batches[0], sc.now)
    b.maps_equal_model()
    n4, n6 = len(b.model.proxy4), len(b.model.proxy6)
    assert proxymap.Flush(b.dp.fd["cilium_proxy4"], b.dp.fd["cilium_proxy6"]) == n4 + n6
    b.model.proxy4.clear(), b.model.proxy6.clear()
    b.maps_equal_model()
    got = b.step(sc.batches[1], sc.now + 1)
    assert not (got["reason"] == 161).any()
    b.maps_equal_model()
    assert set(b.model.proxy4) == keys[1] and _count(b.dp.fd["cilium_proxy4"]) == len(keys[1])
    b.dp.close()


@pytest.mark.gpu
def test_gpu_sweep_is_ordered_on_its_stream():
    """classify, gf_proxy_gc, classify queued on one non-default stream with no
    synchronisation in between: the maps end as the three steps in sequence leave them
    (batch 0's entries are all below the cutoff, batch 1's are not)."""
    _gpu()
    from cilium_amd.datapath import DeviceBatch, ING_OUT, to_numpy
    sc, off = proxy_scenario()
    run = Run(sc, off)
    want0 = run.expect(sc.batches[0], sc.now)
    n4, n6 = len(run.model.proxy4), len(run.model.proxy6)
    run.model.proxy4.clear(), run.model.proxy6.clear()  # the sweep between the batches takes all of batch 0's entries
    want1 = run.expect(sc.batches[1], sc.now + 1)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        io0 = run.dp.ingress(DeviceBatch(sc.batches[0]), sc.now)
        d4 = run.dp.proxy_gc("cilium_proxy4", sc.now + 721)
        d6 = run.dp.proxy_gc("cilium_proxy6", sc.now + 721)
        io1 = run.dp.ingress(DeviceBatch(sc.batches[1]), sc.now + 1)
    s.synchronize()
    assert (d4, d6) == (n4, n6) and n4 > 20 and n6 > 5
    assert np.array_equal(to_numpy(io0, ING_OUT), want0) and np.array_equal(to_numpy(io1, ING_OUT), want1)
    run.maps_equal_model()
    run.dp.close()
