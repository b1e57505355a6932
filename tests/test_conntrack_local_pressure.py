"""Per-endpoint CT maps (the ConntrackLocal endpoint option) under pressure: the states
tests/test_conntrack_local.py never reaches with anything at stake.

libgpuflow decides per call and family how CT inserts are counted (include/gpuflow.h,
"Element accounting of a classify call"): while count + per_pkt * n stays within a map's
insert limit the lanes insert freely and add their net inserts to their program's map
afterwards (non-strict), else every insert is counted exactly (strict; an egress batch
then runs one packet at a time).  Every eviction test of test_conntrack_local.py is
strict by its batch size alone.  Here:

  A  non-strict ingress with eviction, CT4 and CT6 (the kind-1 and kind-2 multi-map
     chains), a synchronise after every call and all calls queued
  B  calls whose sizes straddle the limit: non-strict, strict, non-strict
  C  egress with small per-endpoint maps: strict, mixed with shared maps, non-strict
  D  more than 32 evicting CT6 maps in one call (the 32 + 8 chain split)
  E  per-endpoint HASH CT maps that fill: DROP_CT_CREATE_FAILED at the oracle's packet
  F  in A, C and D every local map's eviction log equals the oracle's

Which path a call must take is asserted from the ORACLE's counts (assert_mode): the
library's bound may be a readback away from the oracle's count but never on the other
side of the limit.  The shapes are the smallest that reach each state (tuned on the
oracle alone); what the oracle produced is asserted in each test.
"""

import numpy as np
import pytest

from cilium_amd import synth
from cilium_amd.synth import Packets
from oracle.scenario import OracleDP

HASH, LRU_HASH = 1, 9
DROP_CT_CREATE_FAILED = 155
STAGE_POLICY = 4
ING, EG_PASS, EG_ALL = 2, 3, 5     # inserts charged per packet: handle_policy; from-container; that + its deliveries


# ---------------------------------------------------------------- the documented rule
def pow2ceil(x):
    p = 1
    while p < x:
        p *= 2
    return p


def insert_limit(kind, max_entries):
    """include/gpuflow.h: an LRU CT map takes inserts up to the 7/8 load of its slot
    array, a power of two >= max(64, 8 x max_entries) for ipv4_ct_tuple ("ct4") and
    4 x for ipv6_ct_tuple ("ct6"); a HASH map ("hash") up to max_entries."""
    if kind == "hash":
        return max_entries
    return pow2ceil(max(64, {"ct4": 8, "ct6": 4}[kind] * max_entries)) // 8 * 7


def map_kind(spec):
    if spec.type != LRU_HASH:
        return "hash"
    return "ct4" if spec.ksz == 14 else "ct6"


def ct_names(sc):
    """Every CT map the scenario's programs bind, each once."""
    out = []
    for e in sc.lxc:
        for fam in ("ct4", "ct6"):
            if e.get(fam) and e[fam] not in out:
                out.append(e[fam])
    return out


def assert_mode(ref, names, n, per_pkt, want_strict):
    """The reference-side condition of a call of n packets over the maps `names`, from
    the oracle's entry counts before it: count + per_pkt * n <= limit for every map
    (non-strict) or not for at least one (strict).  Returns the maps over their limit."""
    over = []
    for name in names:
        spec = ref.sc.maps[name]
        if ref.m[name].count() + per_pkt * n > insert_limit(map_kind(spec), spec.max_entries):
            over.append(name)
    if want_strict:
        assert over, f"a call of {n} packets x {per_pkt} should put some map over its insert limit"
    else:
        assert not over, f"a call of {n} packets x {per_pkt} puts {over} over their insert limits"
    return over


# ---------------------------------------------------------------- comparisons
def diff_records(got, want):
    """Indices of the records that differ (structured arrays of one dtype)."""
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape)
    return np.nonzero(got != want)[0]


def diff_maps(got, want, names):
    """Names of the maps whose dumps differ; got / want: name -> {key: value}."""
    return [n for n in names if got(n) != want(n)]


def check_records(got, want, what):
    bad = diff_records(got, want)
    assert len(bad) == 0, f"{what}: {len(bad)} records differ, first {bad[:1]}"


def check_maps(dp, ref, names):
    bad = diff_maps(dp.dump_map, ref.dump, names)
    assert not bad, f"maps differ: {bad}"


def check_evict_logs(dp, ref, names):
    """F: each LRU map's device log (seq, now_sec, age_cut, hand_line, lines, evicted)
    against the oracle's."""
    from cilium_amd.maps import ctmap
    for n in names:
        if n in ref.lru_log:
            want = [tuple(int(x) for x in e) for e in ref.lru_log[n]]
            assert ctmap.EvictLog(dp.fd[n]) == want, n


def v6_only(pk):
    m = (pk.frames[:, 12] == 0x86) & (pk.frames[:, 13] == 0xdd)
    f = lambda x: None if x is None else x[m]
    return Packets(pk.frames[m], pk.lens[m], f(pk.src_identity), f(pk.ifindex), f(pk.lxc_id), f(pk.tc_index),
                   f(pk.flow_hash))


def concat(pks):
    c = lambda xs: None if xs[0] is None else np.concatenate(xs)
    return Packets(*[c([getattr(p, a) for p in pks]) for a in ("frames", "lens", "src_identity", "ifindex", "lxc_id",
                                                               "tc_index", "flow_hash")])


def calls_of(pk, sizes):
    """pk cut into consecutive calls of the given sizes."""
    out, a = [], 0
    for n in sizes:
        assert a + n <= pk.n, (a, n, pk.n)
        out.append(pk.slice(a, a + n))
        a += n
    return out


def evicting_calls(ref, names):
    """name -> the calls (1-based seq) on which the oracle evicted from it."""
    return {n: [e[0] for e in ref.lru_log[n]] for n in names if ref.lru_log.get(n)}


# ---------------------------------------------------------------- scenarios
def scenario_a(fam):
    """fuzz with every 4th endpoint on small local maps, as many small calls: (sc, made,
    calls).  CT6: the IPv6 rows only, so that the ct6_<id> maps fill."""
    if fam == "ct4":
        sc = synth.fuzz(seed=31, n_packets=15000, n_batches=1)
        made = synth.conntrack_local(sc, every=4, max_entries=160)
        calls = calls_of(sc.batches[0], [300] * 50)
    else:
        sc = synth.fuzz(seed=32, n_packets=20000, n_batches=3)
        made = synth.conntrack_local(sc, every=4, max_entries=100)
        pk = concat([v6_only(b) for b in sc.batches])
        calls = calls_of(pk, [150] * (pk.n // 150))
    return sc, made, calls


def scenario_b():
    """The boundary: calls of 300, one whose 2n alone is just over the ct4_<id> maps'
    limit (897: 1794 > 1792 for max_entries 160), 300s, one just over the ct6_<id> maps'
    (449: 898 > 896), 300s: (sc, made, calls, the two strict calls)."""
    sc = synth.fuzz(seed=33, n_packets=15000, n_batches=1)
    made = synth.conntrack_local(sc, every=4, max_entries=160)
    sizes = [300] * 20 + [897] + [300] * 10 + [449] + [300] * 10
    return sc, made, calls_of(sc.batches[0], sizes), [k for k, n in enumerate(sizes) if n != 300]


EGRESS_CASES = {"every1_small": (1, 60, 500), "every3_small": (3, 60, 500), "every1_mid": (1, 320, 120)}


def scenario_c(case, hazard):
    """egress_fuzz with per-endpoint maps: (sc, made, calls, strict)."""
    every, mx, n = EGRESS_CASES[case]
    sc = synth.egress_fuzz(seed=41 + int(hazard), n_packets=6000, n_batches=1, hazard=hazard)
    made = synth.conntrack_local(sc, every=every, max_entries=mx)
    return sc, made, calls_of(sc.batches[0], [n] * (6000 // n)), case != "every1_mid"


def scenario_d():
    """40 endpoints, each on its own maps, IPv6 rows only."""
    sc = synth.fuzz(seed=34, n_packets=30000, n_batches=3, n_ep=40)
    made = synth.conntrack_local(sc, max_entries=100)
    pk = concat([v6_only(b) for b in sc.batches])
    return sc, made, calls_of(pk, [pk.n // 4] * 4)


def hash_local(sc, made, small, big=100000):
    """E: the local maps as HASH maps, every other endpoint's small, the rest roomy."""
    ids = sorted({int(n.rsplit("_", 1)[1]) for n in made})
    tight = set(ids[::2])
    for n in made:
        m = sc.maps[n]
        m.type = HASH
        m.max_entries = small if int(n.rsplit("_", 1)[1]) in tight else big
        if m.keys is not None and len(m.keys) > m.max_entries:
            m.keys, m.vals = m.keys[:m.max_entries], m.vals[:m.max_entries]
    return tight, set(ids) - tight


def scenario_e(entry):
    """(sc, made, calls, tight, roomy): tight / roomy the lxc ids whose HASH maps are
    small / never fill."""
    if entry == "ingress":
        sc = synth.fuzz(seed=35, n_packets=6000, n_batches=1)
        made = synth.conntrack_local(sc, every=2)
        tight, roomy = hash_local(sc, made, small=150)
        calls = calls_of(sc.batches[0], [400] * 15)
    else:
        sc = synth.egress_fuzz(seed=36, n_packets=3000, n_batches=1, hazard=True)
        made = synth.conntrack_local(sc)
        tight, roomy = hash_local(sc, made, small=100)
        calls = calls_of(sc.batches[0], [300] * 10)
    return sc, made, calls, tight, roomy


def create_failed(recs, pk):
    """lxc id -> DROP_CT_CREATE_FAILED records on that endpoint's maps: the packet's
    endpoint, or for an egress record of stage POLICY the receiver handle_policy ran for."""
    bad = np.nonzero(recs["reason"] == DROP_CT_CREATE_FAILED)[0]
    ep = pk.lxc_id[bad].astype(np.int64)
    if "stage" in recs.dtype.names:
        ep = np.where(recs["stage"][bad] == STAGE_POLICY, recs["lxc_id"][bad], ep)
    ids, cnt = np.unique(ep, return_counts=True)
    return dict(zip(ids.tolist(), cnt.tolist()))


# ---------------------------------------------------------------- CPU: the helper, the shapes, the bite
def test_insert_limit_hand_worked():
    assert insert_limit("ct4", 700) == 7168            # 5600 -> 8192 slots
    assert insert_limit("ct6", 500) == 1792            # 2000 -> 2048
    assert insert_limit("ct4", 64000) == 458752        # 512000 -> 524288
    assert insert_limit("ct6", 64000) == 229376
    assert insert_limit("ct4", 1) == 56 and insert_limit("ct6", 3) == 56      # the 64-slot floor
    assert insert_limit("ct4", 320) == 3584 and insert_limit("ct6", 320) == 1792
    assert insert_limit("hash", 64000) == 64000
    # the egress thresholds include/gpuflow.h states for 64000-entry local maps
    assert 458752 // 3 == 152917 and 64000 // 3 == 21333 and 458752 // 5 == 91750 and 64000 // 5 == 12800


def test_assert_mode_sides():
    sc = synth.fuzz(seed=2, n_packets=64, n_batches=1)
    made = synth.conntrack_local(sc, every=4, max_entries=320)
    ref = OracleDP(sc)
    c4, c6 = ref.m[made[0]].count(), ref.m[made[1]].count()
    assert c4 > 0 and c6 > 0                            # the prefilled entries
    n6 = (1792 - c6) // 2                               # the CT6 maps are the smaller ones
    assert assert_mode(ref, ct_names(sc), n6, ING, False) == []
    over = assert_mode(ref, ct_names(sc), n6 + 1, ING, True)
    assert sorted(over) == sorted(n for n in made if n.startswith("ct6_"))
    with pytest.raises(AssertionError):
        assert_mode(ref, ct_names(sc), n6, ING, True)
    with pytest.raises(AssertionError):
        assert_mode(ref, ct_names(sc), n6 + 1, ING, False)
    assert len(assert_mode(ref, made[:1], (3584 - c4) // 3 + 1, EG_PASS, True)) == 1


def test_comparisons_bite():
    """One byte of one record flipped, one value of one dumped map changed: the helpers
    report exactly that record and that map."""
    sc = synth.fuzz(seed=3, n_packets=500, n_batches=1)
    made = synth.conntrack_local(sc, every=4, max_entries=320)
    ref = OracleDP(sc)
    want = ref.ingress(sc.batches[0], sc.now)
    assert len(diff_records(want.copy(), want)) == 0
    got = want.copy()
    got.view(np.uint8).reshape(len(got), -1)[137, 2] ^= 0x01
    assert list(diff_records(got, want)) == [137]
    with pytest.raises(AssertionError, match="1 records differ"):
        check_records(got, want, "flipped")
    names = ct_names(sc)
    dumps = {n: dict(ref.dump(n)) for n in names}
    assert diff_maps(dumps.__getitem__, ref.dump, names) == []
    victim = next(n for n in made if len(dumps[n]))
    k = sorted(dumps[victim])[0]
    v = bytearray(dumps[victim][k])
    v[0] ^= 0x80
    dumps[victim][k] = bytes(v)
    assert diff_maps(dumps.__getitem__, ref.dump, names) == [victim]
    del dumps[victim][k]                                # a missing entry as well
    assert diff_maps(dumps.__getitem__, ref.dump, names) == [victim]


def test_fuzz_default_endpoints_unchanged():
    """n_ep = 16 is the default and draws nothing extra; more endpoints repeat the flag sets."""
    a, b = synth.fuzz(seed=9, n_packets=300, n_batches=1), synth.fuzz(seed=9, n_packets=300, n_batches=1, n_ep=16)
    assert np.array_equal(a.batches[0].frames, b.batches[0].frames) and a.lxc == b.lxc
    c = synth.fuzz(seed=9, n_packets=300, n_batches=1, n_ep=40)
    assert len(c.lxc) == 40 and c.lxc[16 + 10]["flags"] == c.lxc[10]["flags"]


# ---------------------------------------------------------------- the drivers
# Each runs the oracle over a scenario's calls and asserts, from the oracle alone, that the
# targeted state was reached; with a device datapath (gpu=True) it runs every call there
# too and compares records after each call and maps and eviction logs at the end.
def end_names(sc, made):
    shared = [n for n in ct_names(sc) + ["ct4", "ct6"] if n not in made]
    pol = [f"pol{e}" for e in range(len(sc.lxc))]
    return made + sorted(set(shared)) + pol + [n for n in ("cilium_proxy4", "cilium_proxy6") if n in sc.maps]


def run_ingress(sc, made, calls, strict_calls, gpu, queued=False):
    """strict_calls: the calls (0-based) that must be strict, every other one non-strict.
    queued: every device call enqueued before the first result is looked at."""
    ref, names = OracleDP(sc), ct_names(sc)
    if gpu:
        import torch
        from cilium_amd.datapath import Datapath, DeviceBatch, ING_OUT, to_numpy
        dp = Datapath(sc, pin_prefix=None)
        dbs = [DeviceBatch(pk) for pk in calls]
        torch.cuda.synchronize()
        outs = []
        if queued:
            outs = [dp.ingress(db, sc.now + k) for k, db in enumerate(dbs)]
            torch.cuda.synchronize()
    for k, pk in enumerate(calls):
        assert_mode(ref, names, pk.n, ING, k in strict_calls)
        want = ref.ingress(pk, sc.now + k)
        if gpu:
            if not queued:
                outs.append(dp.ingress(dbs[k], sc.now + k))
                torch.cuda.synchronize()
            check_records(to_numpy(outs[k], ING_OUT), want, f"call {k}")
    if gpu:
        check_maps(dp, ref, end_names(sc, made))
        check_evict_logs(dp, ref, made)
        dp.close()
    return ref


def run_egress(sc, made, calls, strict, gpu):
    ref, names = OracleDP(sc), ct_names(sc)
    failed, filled = {}, set()
    if gpu:
        import torch
        from cilium_amd.datapath import Datapath, DeviceBatch, EG_OUT, to_numpy
        dp = Datapath(sc, pin_prefix=None)
    for k, pk in enumerate(calls):
        if strict:
            assert_mode(ref, names, pk.n, EG_PASS, True)
        else:
            assert_mode(ref, names, pk.n, EG_ALL, False)
        ro, rs = ref.egress(pk, sc.now + k)
        for ep, c in create_failed(ro, pk).items():
            failed[ep] = failed.get(ep, 0) + c
        filled |= full_endpoints(ref, made)
        if gpu:
            out, snap = dp.egress(DeviceBatch(pk, parse=False), sc.now + k)
            torch.cuda.synchronize()
            check_records(to_numpy(out, EG_OUT), ro, f"egress call {k}")
            assert not (snap.cpu().numpy() != rs).any(), f"frames of call {k}"
    if gpu:
        check_maps(dp, ref, end_names(sc, made))
        check_evict_logs(dp, ref, made)
        dp.close()
    return ref, failed, filled


def full_endpoints(ref, made):
    """The lxc ids with a HASH map of their own at max_entries."""
    return {int(n.rsplit("_", 1)[1]) for n in made
            if ref.sc.maps[n].type == HASH and ref.m[n].count() >= ref.sc.maps[n].max_entries}


def drive_a(fam, queued, gpu):
    sc, made, calls = scenario_a(fam)
    ref = run_ingress(sc, made, calls, (), gpu, queued)
    ev = evicting_calls(ref, [n for n in made if n.startswith(fam + "_")])
    assert len(ev) >= 2, ev                             # two local maps of the family evicted,
    assert max(len(set(v)) for v in ev.values()) >= 2, ev   # one of them on two different calls
    return {"calls": len(calls), "strict": [], "maps_evicting": len(ev), "evictions": sum(len(v) for v in ev.values())}


def drive_b(queued, gpu):
    sc, made, calls, big = scenario_b()
    ref = run_ingress(sc, made, calls, big, gpu, queued)
    ev = evicting_calls(ref, [n for n in made if n.startswith("ct4_")])
    seqs = sorted({s for v in ev.values() for s in v})  # 1-based calls with a CT4 eviction
    # evictions before the first strict call, between the two and after the last: the counts the
    # non-strict calls accumulate reach the strict one, and the strict call's the ones after it
    assert any(s <= big[0] for s in seqs) and any(big[0] + 1 < s <= big[1] for s in seqs) and \
        any(s > big[1] + 1 for s in seqs), (big, seqs)
    return {"calls": len(calls), "strict": big, "maps_evicting": len(ev), "evictions": sum(len(v) for v in ev.values())}


def drive_c(case, hazard, gpu):
    sc, made, calls, strict = scenario_c(case, hazard)
    ref, failed, _ = run_egress(sc, made, calls, strict, gpu)
    own4 = [n for n in made if n.startswith("ct4_")]
    assert [n for n in own4 if len(ref.dump(n))], "the senders' own maps should hold their connections"
    ev = evicting_calls(ref, own4)
    assert 2 * len(ev) > len(own4), (len(ev), len(own4))    # a majority of the ct4_* maps evicted
    assert sum(len(set(v)) > 1 for v in ev.values()) >= 2, ev   # over several calls
    assert not failed, failed
    return {"calls": len(calls), "strict": list(range(len(calls))) if strict else [], "maps_evicting": len(ev),
            "of": len(own4), "evictions": sum(len(v) for v in ev.values())}


def drive_d(gpu):
    sc, made, calls = scenario_d()
    assert len(made) == 80
    ref = run_ingress(sc, made, calls, range(len(calls)), gpu)
    ev = evicting_calls(ref, [n for n in made if n.startswith("ct6_")])
    per_call = [sum(k + 1 in v for v in ev.values()) for k in range(len(calls))]
    assert max(per_call) > 32, per_call                 # more maps than one chain takes (GF_LRU_MULTI = 32)
    return {"calls": len(calls), "strict": list(range(len(calls))), "maps_evicting": len(ev), "per_call": per_call}


def drive_e(entry, gpu):
    sc, made, calls, tight, roomy = scenario_e(entry)
    if entry == "ingress":
        ref, names = OracleDP(sc), ct_names(sc)
        failed, filled = {}, set()
        if gpu:
            import torch
            from cilium_amd.datapath import Datapath, DeviceBatch, ING_OUT, to_numpy
            dp = Datapath(sc, pin_prefix=None)
        for k, pk in enumerate(calls):
            assert_mode(ref, names, pk.n, ING, True)
            want = ref.ingress(pk, sc.now + k)
            for ep, c in create_failed(want, pk).items():
                failed[ep] = failed.get(ep, 0) + c
            filled |= full_endpoints(ref, made)
            if gpu:
                io = dp.ingress(DeviceBatch(pk), sc.now + k)
                torch.cuda.synchronize()
                check_records(to_numpy(io, ING_OUT), want, f"call {k}")
        if gpu:
            check_maps(dp, ref, end_names(sc, made))
            dp.close()
    else:
        ref, failed, filled = run_egress(sc, made, calls, True, gpu)
    # DROP_CT_CREATE_FAILED on at least two endpoints, only on endpoints whose own map filled
    assert len(failed) >= 2 and set(failed) <= filled <= tight and not set(failed) & roomy, (failed, filled)
    return {"calls": len(calls), "strict": list(range(len(calls))), "create_failed": sum(failed.values()),
            "endpoints_failed": len(failed), "maps_full": len(filled)}


def test_shapes_reach_their_states():
    """CPU: every scenario against the oracle alone: the mode of each call, the evictions
    and the failed inserts each GPU test below relies on."""
    for fam in ("ct4", "ct6"):
        drive_a(fam, False, False)
    drive_b(False, False)
    for case in EGRESS_CASES:
        for hazard in (True, False):
            drive_c(case, hazard, False)
    drive_d(False)
    for entry in ("ingress", "egress"):
        drive_e(entry, False)


# ---------------------------------------------------------------- GPU parity
torch = pytest.importorskip("torch")


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(0)


@pytest.mark.gpu
@pytest.mark.parametrize("queued", [False, True], ids=["synced", "queued"])
@pytest.mark.parametrize("fam", ["ct4", "ct6"])
def test_gpu_nonstrict_ingress_evicts(fam, queued):
    """A, F: every 4th endpoint on small maps of its own, 50 calls none of which can put
    a map over its insert limit (non-strict: each lane adds its net inserts to its
    program's map), the maps evicting again and again through the multi-map pass (kind 1
    for ct4; kind 2 for ct6, fed IPv6 rows only).  queued: no host sync between the
    calls, so the host's bounds follow only the stamps of the eviction passes.  Records
    of every call, every map and each local map's eviction log equal the oracle's."""
    _gpu()
    drive_a(fam, queued, True)


@pytest.mark.gpu
@pytest.mark.parametrize("queued", [False, True], ids=["synced", "queued"])
def test_gpu_strict_boundary(queued):
    """B: calls of 300 packets (non-strict), one of 897 (2n = 1794 > 1792, the ct4_<id>
    maps' limit: both families strict), 300s again, one of 449 (2n = 898 > 896, the
    ct6_<id> maps': family 6 only), 300s again, with evictions in every stretch: the
    counts carry across the flips in both directions."""
    _gpu()
    drive_b(queued, True)


@pytest.mark.gpu
@pytest.mark.parametrize("hazard", [True, False], ids=["hazard", "nohazard"])
@pytest.mark.parametrize("case", list(EGRESS_CASES))
def test_gpu_egress_pressure(case, hazard):
    """C, F: from-container and its deliveries over small per-endpoint maps: every
    sender's map evicting with every call strict (3n alone over the limit: the batch runs
    one packet at a time), every 3rd endpoint local and the rest shared, and maps sized
    so that no call is strict (count + 5n within the limit) and the service entries'
    count adds land on maps at their high-water mark.  Records, rewritten frames, every
    CT map, policy counters, proxy maps and eviction logs equal the oracle's."""
    _gpu()
    drive_c(case, hazard, True)


@pytest.mark.gpu
def test_gpu_many_ct6_maps_evict():
    """D, F: 40 endpoints with IPv6 traffic on maps of their own: more than 32 ct6_<id>
    maps evict in one call, two chains of the kind-2 multi-map pass (32 + the rest)."""
    _gpu()
    drive_d(True)


@pytest.mark.gpu
@pytest.mark.parametrize("entry", ["ingress", "egress"])
def test_gpu_hash_local_maps_fill(entry):
    """E: per-endpoint HASH CT maps, every other one small: an insert fails with
    DROP_CT_CREATE_FAILED at exactly max_entries, at the oracle's packet, on the endpoints
    whose map filled and on no other."""
    _gpu()
    drive_e(entry, True)
