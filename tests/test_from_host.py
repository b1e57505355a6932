"""The from-host entry point — gf_host_classify (bpf/bpf_netdev.c compiled with -DFROM_HOST,
the program on cilium_host): the proxy's identity from skb->mark, the reverse translation out
of cilium_proxy4 / 6, rewrite_dmac_to_host, endpoint lookup, local delivery into the
cilium_policy tail call, and encap_and_redirect for remote pods.

The CPU oracle cannot express FROM_HOST.  The checks rest on:

 1. hand-derived known answers (tests/golden/from_host_kats.json; every expected checksum is a
    full recomputation over the rewritten frame);
 2. coincidence with from_netdev: with every mark 0, empty proxy maps and ENCAP_IFINDEX
    undefined the program is from_netdev with the same FIXED_SRC_SECCTX except for
    rewrite_dmac_to_host — OracleDP.pipeline without XDP / LB, stage 3 renamed 7, trace subtype
    8 renamed 7 with src_label HOST_ID;
 3. tests/host_model.py, a per-packet restatement of the front from the reference, followed by
    OracleDP.ingress (or tests/ctoff_model.py) over the delivered subset in batch order.

Frames: handle_policy itself writes frames and OracleDP.ingress returns none, so against the
model the frames of stage-7 packets (always, in full) and of IPv4 deliveries forwarded as
CT_NEW / CT_ESTABLISHED without a proxy redirect are compared (as tests/test_overlay.py).
"""
import copy
import errno
import json
import os
import struct

import numpy as np
import pytest

import oracle.oracle as O
from cilium_amd import synth
from cilium_amd.synth import Packets
from oracle.scenario import OracleDP
from tests import ctoff_model as CM
from tests import host_model as HM
from tests.overlay_model import PIPE_OUT

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KAT_NOW = 5000
NET_MAC = bytes.fromhex("02c1110e7001")
FUZZ = [(3, "plain"), (4, "local"), (5, "ctoff")]       # the batches the GPU fuzz cases use
KAT_NAMES = {"mark_none", "mark_fea_identity", "mark_fea_no_identity", "mark_feb_identity", "mark_near_miss", "fixed_secctx",
             "fixed_secctx_overridden", "rev_hit_tcp4", "rev_hit_udp4_csum", "rev_hit_udp4_zero_csum", "rev_miss_tcp4",
             "icmp4_ignored", "rev_hit_tcp6", "rev_hit_udp6", "rev_miss_tcp6", "v6_exthdr_ignored", "v6_derived_secctx",
             "v6_world_secctx", "ports_not_loadable", "v4_len33", "v6_len53", "arp", "endpoint_host", "v4_ttl1", "v6_hop1",
             "portmap_delivery", "missing_policy_slot", "encap_v4_hit", "encap_ifindex_0", "encap_tunnel_miss",
             "encap_outside_cluster", "encap_v6_hit"}


def _subset(pk, m):
    f = lambda x: None if x is None else x[m]
    return Packets(pk.frames[m], pk.lens[m], f(pk.src_identity), f(pk.ifindex), f(pk.lxc_id), f(pk.tc_index),
                   f(pk.flow_hash), None, f(pk.mark))


# ---------------------------------------------------------------- KATs
def _kats():
    with open(os.path.join(GOLDEN, "from_host_kats.json")) as f:
        return json.load(f)["cases"]


def kat_scenario(variant):
    """The KATs of one variant as one batch (A: ENCAP_IFINDEX undefined, no FIXED_SRC_SECCTX;
    B: ENCAP_IFINDEX 9, FIXED_SRC_SECCTX 300).  Returns (scenario, cases, expected records,
    expected frames)."""
    cases = [c for c in _kats() if c["variant"] == variant]
    sc = synth.Scenario(f"host_kats{variant}", now=KAT_NOW, host_ifindex=3)
    mac = lambda s: np.frombuffer(bytes.fromhex(s), np.uint8)
    a6 = np.frombuffer(bytes.fromhex("f00d" + "00" * 13 + "01"), np.uint8)
    h6 = np.frombuffer(bytes.fromhex("f00d" + "00" * 13 + "fe"), np.uint8)
    ips = ["10.1.0.1", "10.1.0.2", "10.1.0.3", "10.1.0.254"]
    keys = np.concatenate([synth.endpoint_keys4([synth.ip4(a) for a in ips]), synth.endpoint_keys6(np.stack([a6, h6]))])
    vals = synth.endpoint_infos(np.array([11, 12, 13, 1, 11, 1]), np.zeros(6), np.array([3000, 3001, 3002, 0, 3000, 0]),
                                np.array([0, 0, 0, 1, 0, 1]))
    for row, (m, nm) in {0: ("aa1111111111", "bb2222222222"), 1: ("aa3333333333", "bb4444444444"),
                         2: ("aa5555555555", "bb6666666666"), 4: ("aa1111111111", "bb2222222222")}.items():
        vals[row, 16:22], vals[row, 24:30] = mac(m), mac(nm)
    vals[1, 48:52] = np.frombuffer(struct.pack(">HH", 80, 8080), np.uint8)   # struct portmap {from, to}
    sc.add_map(synth.MapSpec("cilium_lxc", synth.HASH, 20, 112, 1024, 0, keys, vals))
    sc.add_map(synth.MapSpec("ct4", synth.LRU_HASH, 14, 48, 4096, 0))
    sc.add_map(synth.MapSpec("ct6", synth.LRU_HASH, 40, 48, 4096, 0))
    for k, lid in enumerate((3000, 3001)):
        sc.add_map(synth.MapSpec(f"pol{k}", synth.HASH, 8, 24, 1024, 0, synth.policy_keys([300], [0], [0]),
                                 synth.policy_vals([0])))
        sc.lxc.append({"lxc_id": lid, "seclabel": 500 + k, "policy": f"pol{k}", "ct4": "ct4", "ct6": "ct6",
                       "flags": synth.LXC_PRODUCTION, "l4": []})
    # cilium_proxy4 / 6: {client 10.1.0.1 / f00d::1, dport 15000, sport 40000} -> 10.9.0.9:80 / [f00d::99]:80
    ports, tail = struct.pack(">HH", 15000, 40000), struct.pack(">HH", 80, 0) + struct.pack("<II", 300, KAT_NOW + 600)
    s4, s6 = bytes([10, 9, 0, 9]), bytes.fromhex("f00d" + "00" * 13 + "99")
    k4 = [bytes([10, 1, 0, 1]) + ports + bytes([nh, 0]) for nh in (6, 17)]
    k4.append(bytes([10, 1, 0, 1]) + struct.pack(">HH", 15000, 40001) + bytes([17, 0]))   # a second client port (UDP)
    k6 = [bytes(a6) + ports + bytes([nh, 0]) for nh in (6, 17)]
    u8 = lambda rows: np.frombuffer(b"".join(rows), np.uint8).reshape(len(rows), -1).copy()
    sc.add_map(synth.MapSpec("cilium_proxy4", synth.HASH, 10, 16, 1024, 0, u8(k4), u8([s4 + tail] * 3)))
    sc.add_map(synth.MapSpec("cilium_proxy6", synth.HASH, 22, 28, 1024, 0, u8(k6), u8([s6 + tail] * 2)))
    router = bytes.fromhex("20010db8aabb" + "00" * 10)
    tk = np.concatenate([synth.endpoint_keys4([synth.ip4("10.77.2.0")]),
                         synth.endpoint_keys6(np.frombuffer(router, np.uint8)[None, :])])
    tv = synth.endpoint_keys4([synth.ip4("192.168.9.1"), synth.ip4("192.168.9.2")])
    sc.add_map(synth.MapSpec("cilium_tunnel_map", synth.HASH, 20, 20, 64, 0, tk, tv))
    sc.node = {"proxy4": "cilium_proxy4", "proxy6": "cilium_proxy6", "host_mac": bytes.fromhex("ce72a7038856"),
               "node_mac": bytes.fromhex("deadbeefc0de"), "ipv4_gateway": 0xfffff50a,
               "encap_ifindex": 9 if variant == "B" else 0, "tunnel_map": "cilium_tunnel_map", "router_ip6": router,
               "ipv4_cluster_range": 0x00004d0a, "ipv4_cluster_mask": 0x0000ffff, "ipv4_mask": 0x00ffffff}
    sc.host = {"lxc_map": "cilium_lxc", "flags": 1 if variant == "B" else 0, "fixed_secctx": 300 if variant == "B" else 0,
               "router_ip6": router, "ingress_ifindex": 5, "cilium_net_mac": NET_MAC}
    n, S = len(cases), 128
    frames, lens = np.zeros((n, S), np.uint8), np.zeros(n, np.uint32)
    want, wantf = np.zeros(n, PIPE_OUT), np.zeros((n, S), np.uint8)
    for k, c in enumerate(cases):
        fb = bytes.fromhex(c["frame"])
        frames[k, :len(fb)] = np.frombuffer(fb, np.uint8)
        lens[k] = c["len"]
        wantf[k] = frames[k]
        for off, hx in c["changed"].items():
            b = bytes.fromhex(hx)
            wantf[k, int(off):int(off) + len(b)] = np.frombuffer(b, np.uint8)
        for name, v in c["expect"].items():
            want[k][name] = v
    mark = np.array([c["mark"] for c in cases], np.uint32)
    sc.batches.append(Packets(frames, lens, None, None, None, np.zeros(n, np.uint8), np.zeros(n, np.uint32), None, mark))
    return sc, cases, want, wantf


def model_run(sc, pk, now, ref, model, ctoff=None, off=()):
    """The model's front over the proxy maps as they stand at the start of the call, then
    handle_policy of the delivered subset in batch order: the oracle's, or tests/ctoff_model.py
    for endpoints without conntrack.  Returns (records, front frames, front records, the
    delivered subset's tc_index)."""
    rec, frames, dl, sub = model.front(pk, ref.parse(pk), ref.dump("cilium_proxy4"), ref.dump("cilium_proxy6"))
    ing = np.zeros(sub.n, CM.ING_OUT)
    if sub.n:
        offm = np.isin(sub.lxc_id, list(off)) if ctoff is not None else np.zeros(sub.n, bool)
        if (~offm).any():
            s2 = Packets(sub.frames[~offm], sub.lens[~offm], sub.src_identity[~offm], sub.ifindex[~offm],
                         sub.lxc_id[~offm], sub.tc_index[~offm], None if sub.flow_hash is None else sub.flow_hash[~offm])
            ing[~offm] = ref.ingress(s2, now)
        if offm.any():
            idx, mrec, _ = ctoff.batch(sub, ref.parse(sub), now, mask=offm)
            assert np.array_equal(idx, np.nonzero(offm)[0])
            ing[offm] = mrec
    return HM.complete(rec, dl, ing), frames, rec, (dl, sub)


def test_kats_cover_the_issue_list():
    names = [c["name"] for c in _kats()]
    assert len(names) == len(set(names)) and set(names) == KAT_NAMES and all(c["derivation"] for c in _kats())


def _valid_checksums(row, length):
    """Full recomputation over the frame: the IPv4 header and the TCP / UDP checksum."""
    b = bytes(row[:length])
    fold = lambda x: 0xffff ^ _csum16(x)                # the folded ones-complement sum: 0xffff when valid
    if b[12:14] == b"\x08\x00":
        l4, nh = 14 + (b[14] & 0xf) * 4, b[23]
        if fold(b[14:l4]) != 0xffff:
            return False
        ph = b[26:34] + struct.pack(">BBH", 0, nh, len(b) - l4)
    else:
        l4, nh = 54, b[20]
        ph = b[22:54] + struct.pack(">IHBB", len(b) - l4, 0, 0, nh)
    if nh == 17 and b[l4 + 6:l4 + 8] == b"\0\0":
        return True
    return nh not in (6, 17) or fold(ph + b[l4:]) == 0xffff


@pytest.mark.parametrize("variant", ["A", "B"])
def test_model_reproduces_every_kat(variant):
    sc, cases, want, wantf = kat_scenario(variant)
    ref = OracleDP(sc)
    got, frames, _, _ = model_run(sc, sc.batches[0], sc.now, ref, HM.HostModel(sc))
    for k, c in enumerate(cases):
        assert got[k] == want[k], (c["name"], got[k], want[k])
        assert bytes(frames[k]) == bytes(wantf[k]), c["name"]
        if c["name"].startswith("rev_hit"):             # the KAT's own checksums are whole-frame valid
            assert _valid_checksums(wantf[k], c["len"]), c["name"]


# ---------------------------------------------------------------- coincidence with from_netdev
COINCIDE_T = 260


def coincidence_scenario(seed, n_packets=12000, trace=False):
    """pipeline_fuzz as cilium_host sees it with every mark 0 (mark None), empty proxy maps and
    ENCAP_IFINDEX undefined.  Returns (the from-host scenario, the same scenario as from_netdev
    sees it: no XDP / LB, the same FIXED_SRC_SECCTX)."""
    sc = synth.pipeline_fuzz(seed=seed, n_packets=n_packets, n_batches=3)
    # TCP / UDP frames too short for their 4 port bytes are left out: reverse_proxy ends them with
    # DROP_CT_INVALID_HDR in the front (:280-281), where from_netdev delivers them and handle_policy's
    # conntrack drops them with the same reason (the KAT ports_not_loadable covers the front's drop)
    for bi, pk in enumerate(sc.batches):
        f, ln = pk.frames, pk.lens.astype(np.int64)
        v4 = (f[:, 12] == 0x08) & (f[:, 13] == 0) & (ln >= 34)
        v6 = (f[:, 12] == 0x86) & (f[:, 13] == 0xDD) & (ln >= 54)
        l4 = np.where(v4, 14 + (f[:, 14] & 0xf).astype(np.int64) * 4, 54)
        nh = np.where(v4, f[:, 23], f[:, 20])
        sc.batches[bi] = _subset(pk, ~((v4 | v6) & np.isin(nh, (6, 17)) & (l4 + 4 > ln)))
    if trace:
        for k, e in enumerate(sc.lxc):
            if k % 3 == 0:
                e["flags"] |= synth.LXC_TRACE_NOTIFY
    flags = 1 | (synth.NETDEV_TRACE_NOTIFY if trace else 0)
    sc.host = dict(sc.netdev, flags=flags, fixed_secctx=COINCIDE_T, ingress_ifindex=9, cilium_net_mac=NET_MAC)
    nd = copy.copy(sc)
    nd.xdp = nd.lb = None
    nd.netdev = dict(sc.netdev, flags=flags, fixed_secctx=COINCIDE_T, ingress_ifindex=9)
    return sc, nd


def renamed(ro):
    ro = ro.copy()
    ro["stage"][ro["stage"] == 3] = HM.STAGE_HOST
    return ro


def _coincidence_frames(pk, want, rs):
    """The oracle's from_netdev frames as from-host leaves them: bytes 0-5 = CILIUM_NET_MAC for
    the IP packets that end in the front after rewrite_dmac_to_host, which are those from_netdev
    ends without its local delivery having stored MACs (a delivery that fails in map_lxc_in has
    stored them, over CILIUM_NET_MAC).  Returns (frames, that mask)."""
    ip = ((pk.frames[:, 12] == 0x08) & (pk.frames[:, 13] == 0) & (pk.lens >= 34)) | \
         ((pk.frames[:, 12] == 0x86) & (pk.frames[:, 13] == 0xDD) & (pk.lens >= 54))
    m = (want["stage"] == 7) & ip & (rs[:, 0:12] == pk.frames[:, 0:12]).all(axis=1)
    rs = rs.copy()
    rs[m, 0:6] = np.frombuffer(NET_MAC, np.uint8)
    return rs, m


def _frames_cmp(pk, want):
    """Packets whose frame handle_policy does not write (see the module docstring)."""
    return (want["stage"] == 7) | ((pk.frames[:, 12] == 0x08) & (want["flags"] & 1 == 0) & (want["action"] != 2) &
                                   (want["ct_ret"] < 2))


def test_model_against_oracle_on_coincidence_batch():
    """Ties the model to the oracle: the model's front + OracleDP.ingress equals
    OracleDP.pipeline (from_netdev with the same FIXED_SRC_SECCTX), stage 3 renamed 7."""
    sc, nd = coincidence_scenario(3, n_packets=4000)
    ref, pipe, model = OracleDP(sc), OracleDP(nd), HM.HostModel(sc)
    seen = set()
    for bi, pk in enumerate(sc.batches):
        got, frames, front, _ = model_run(sc, pk, sc.now + bi, ref, model)
        ro, _, rs = pipe.pipeline(pk, sc.now + bi)
        want = renamed(ro)
        bad = np.nonzero(got != want)[0]
        assert len(bad) == 0, f"b{bi}: {len(bad)} differ, first {bad[:1]}: {got[bad[:1]]} != {want[bad[:1]]}"
        rs, dm = _coincidence_frames(pk, want, rs)
        assert dm.any() and (frames[dm, 0:6] == np.frombuffer(NET_MAC, np.uint8)).all()
        cmp = _frames_cmp(pk, want)
        assert cmp.sum() > pk.n // 3 and not (frames[cmp] != rs[cmp]).any(), f"frames b{bi}"
        seen |= set(zip(want["stage"].tolist(), want["action"].tolist()))
    for name in ["ct4", "ct6", "cilium_proxy4", "cilium_proxy6"] + [e["policy"] for e in sc.lxc]:
        assert ref.dump(name) == pipe.dump(name), name
    assert {(4, 7), (4, 2), (7, 0), (7, 2), (7, 7)} <= seen, seen


# ---------------------------------------------------------------- host_fuzz
def fuzz_scenario(seed, kind, n_packets=20000 // 3, n_batches=3):
    sc = synth.host_fuzz(seed=seed, n_packets=n_packets, n_batches=n_batches)
    off = []
    if kind == "local":
        synth.conntrack_local(sc, every=2)
    elif kind == "ctoff":
        off = synth.conntrack_off(sc, every=2)
        for e in sc.lxc:                                # cilium_proxy4 / 6 are shared with the CT-on half
            if e["lxc_id"] in off:
                sc.maps[e["policy"]].vals[:, 0:2] = 0
    return sc, off


@pytest.mark.parametrize("seed,kind", FUZZ)
def test_host_fuzz_is_not_thin(seed, kind):
    """Every batch the GPU fuzz cases use shows, by the model and the reference alone: stages 4
    and 7, reverse hits for v4 and v6, both mark magics, skip-proxy packets that a proxy rule
    would otherwise have redirected, an encap redirect and a tunnel miss, policy allows and
    denies, CT entries created, a drop at the front, an ICMP6_TE, and no class above 60 %."""
    sc, off = fuzz_scenario(seed, kind)
    ref, model = OracleDP(sc), HM.HostModel(sc)
    ctoff = CM.CtOffModel(sc) if off else None
    t4 = {bytes(k[:4]) for k in sc.maps["cilium_tunnel_map"].keys if k[16] == 1}
    for bi, pk in enumerate(sc.batches):
        # the same state without the program's SKIP_PROXY bits: a second oracle replays the
        # earlier batches, then this one with tc_index as it came
        probe, pm = OracleDP(sc), HM.HostModel(sc)
        pco = CM.CtOffModel(sc) if off else None
        for bj in range(bi):
            model_run(sc, sc.batches[bj], sc.now + bj, probe, pm, pco, off)
        prec, _, pdl, psub = pm.front(pk, probe.parse(pk), probe.dump("cilium_proxy4"), probe.dump("cilium_proxy6"))
        ct_on = ~np.isin(psub.lxc_id, list(off))
        noskip = Packets(psub.frames[ct_on], psub.lens[ct_on], psub.src_identity[ct_on], psub.ifindex[ct_on],
                         psub.lxc_id[ct_on], pk.tc_index[pdl][ct_on], psub.flow_hash[ct_on])
        pin = probe.ingress(noskip, sc.now + bi)
        got, _, front, (dl, sub) = model_run(sc, pk, sc.now + bi, ref, model, ctoff, off)
        assert np.array_equal(dl, pdl)
        skipped = ((sub.tc_index[ct_on] & 1) != 0) & ((pk.tc_index[pdl][ct_on] & 1) == 0)
        assert (skipped & (pin["flags"] & 1 != 0) & (got["flags"][dl][ct_on] & 1 == 0)).any(), "skip-proxy effect"
        v4, v6 = pk.frames[:, 12] == 0x08, pk.frames[:, 12] == 0x86
        s4, s7 = got["stage"] == 4, got["stage"] == 7
        rev = got["flags"] & 0x10 != 0
        assert s4.any() and s7.any() and (rev & v4).any() and (rev & v6).any()
        magic = pk.mark & 0xFFF
        assert (magic == 0xFEA).any() and (magic == 0xFEB).any()
        enc = s7 & (got["action"] == 7) & (got["ifindex_lo"] == 7) & (got["daddr4"] != 0)
        in_cluster = v4 & (pk.lens >= 34) & (pk.frames[:, 30] == 10) & (pk.frames[:, 31] == 77)
        miss = in_cluster & s7 & (got["action"] == 0) & \
            np.array([bytes(r[30:33]) + b"\0" not in t4 for r in pk.frames])
        assert (enc & v4).any() and (enc & v6).any() and miss.any()
        assert (s4 & (got["action"] != 2)).any() and (s4 & (got["reason"] == 133)).any()
        assert (s4 & (got["flags"] & 2 != 0)).any(), "CT created"
        assert (s7 & (got["action"] == 2)).any(), "a drop at the front"
        assert (s7 & (got["flags"] & 0x20 != 0)).any(), "ICMP6_TE"
        classes = {"delivered": s4, "encap": enc, "front_drop": s7 & (got["action"] == 2), "stack": s7 & (got["action"] == 0),
                   "reverse": rev}
        for name, m in classes.items():
            assert m.sum() * 10 <= pk.n * 6, (name, int(m.sum()), pk.n)


# ---------------------------------------------------------------- error returns without a device
def test_host_load_errors():
    import ctypes as C
    from cilium_amd import bpf
    from cilium_amd._lib import lib, gf_host_cfg, gf_host_batch, gf_netdev_cfg, gf_frames
    cfg = lambda lxc, arr: gf_host_cfg(gf_netdev_cfg(lxc, 0, 0, (C.c_uint8 * 16)(), 5), (C.c_uint8 * 6)(*NET_MAC), arr)
    assert lib.gf_host_load(None) == -errno.EFAULT
    assert lib.gf_host_load(C.byref(cfg(987654, 987655))) == -errno.EBADF
    good = bpf.CreateMap(synth.HASH, 20, 112, 64, 0)
    wrong = bpf.CreateMap(synth.HASH, 20, 104, 64, 0)
    arr = lib.gf_policy_array_create()
    try:
        assert lib.gf_host_load(C.byref(cfg(wrong, arr))) == -errno.EINVAL    # not endpoint_info
        assert lib.gf_host_load(C.byref(cfg(good, good))) == -errno.EBADF     # not a prog array
        assert lib.gf_host_load(C.byref(cfg(arr, arr))) == -errno.EBADF       # not a map
        host = lib.gf_host_load(C.byref(cfg(good, arr)))
        assert host > 0
        b = gf_host_batch()
        assert lib.gf_host_classify(good, C.byref(b), 0, None, None, None) == -errno.EBADF    # not a from-host program
        assert lib.gf_host_classify(987654, C.byref(b), 0, None, None, None) == -errno.EBADF
        assert lib.gf_host_classify(host, None, 0, None, None, None) == -errno.EFAULT
        assert lib.gf_host_classify(host, C.byref(b), 0, None, None, None) == 0               # n == 0
        b = gf_host_batch(gf_frames(4, 64, None, None), None, None, None)
        assert lib.gf_host_classify(host, C.byref(b), 0, None, None, None) == -errno.EFAULT   # NULL frames
        # the argument checks come before any device work: host buffers stand in for the pointers
        buf = (C.c_uint8 * 4096)()
        p = C.addressof(buf)
        for n, stride, want in ((4, 13, -errno.EINVAL), (4, 257, -errno.EINVAL), ((1 << 30) + 1, 64, -errno.E2BIG)):
            b = gf_host_batch(gf_frames(n, stride, p, p), None, None, None)
            assert lib.gf_host_classify(host, C.byref(b), 0, p, None, None) == want, (n, stride)
        b = gf_host_batch(gf_frames(4, 64, p, p), None, None, None)
        assert lib.gf_host_classify(host, C.byref(b), 0, None, None, None) == -errno.EFAULT   # NULL out
        bpf.ObjClose(host)
    finally:
        for h in (arr, good, wrong):
            bpf.ObjClose(h)


def test_packets_mark_is_the_last_field():
    f, ln = np.zeros((3, 64), np.uint8), np.full(3, 60, np.uint32)
    pk = Packets(f, ln, None, None, None, None, None, np.arange(3, dtype=np.uint32))   # positional, as before
    assert pk.mark is None and pk.tunnel_id[2] == 2
    pk = Packets(f, ln, mark=np.array([1, 2, 3], np.uint32))
    assert pk.slice(1, 3).mark.tolist() == [2, 3]


# ---------------------------------------------------------------- GPU
torch = pytest.importorskip("torch")


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(0)


def _gpu_host(dp, pk, now, snap_out=True, bare=False):
    from cilium_amd.datapath import DeviceBatch, to_numpy
    b = DeviceBatch(pk, parse=False)
    if bare:
        b.tc_index = b.flow_hash = b.mark = None
    out, snap = dp.from_host(b, now, snap_out=snap_out)
    torch.cuda.synchronize()
    return to_numpy(out, PIPE_OUT), None if snap is None else snap.cpu().numpy()


def _frames_same(snap, frames, cmp, want, what):
    bad = np.nonzero(cmp & (snap != frames).any(axis=1))[0]
    if len(bad):
        i = bad[0]
        off = np.nonzero(snap[i] != frames[i])[0]
        raise AssertionError(f"{what}: {len(bad)} frames differ, first {i} {want[i]} at offsets {off[:12]}: "
                             f"{bytes(snap[i][off[:12]]).hex()} != {bytes(frames[i][off[:12]]).hex()}; frame {bytes(frames[i][:64]).hex()}")


def _same(got, want, what):
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, f"{what}: {len(bad)} records differ, first {bad[:1]}: {got[bad[:1]]} != {want[bad[:1]]}"


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["A", "B"])
def test_gpu_kats(variant):
    """The KATs on the device: ENCAP_IFINDEX undefined (A) and 9 (B)."""
    _gpu()
    from cilium_amd.datapath import Datapath
    sc, cases, want, wantf = kat_scenario(variant)
    dp = Datapath(sc, pin_prefix=None)
    before = (dp.dump_map("cilium_proxy4"), dp.dump_map("cilium_proxy6"))
    got, snap = _gpu_host(dp, sc.batches[0], sc.now)
    for k, c in enumerate(cases):
        assert got[k] == want[k], (c["name"], got[k], want[k])
        assert bytes(snap[k]) == bytes(wantf[k]), c["name"]
    assert (dp.dump_map("cilium_proxy4"), dp.dump_map("cilium_proxy6")) == before
    dp.close()


def _event(w0, length, w4, w5, w6, w7, payload):
    """One 160-B ring record: 8 header words (hash 0), then the first min(len, 128) payload bytes."""
    cap = min(length, 128)
    r = np.zeros(160, np.uint8)
    r[:32] = np.frombuffer(struct.pack("<8I", w0, 0, length, cap, w4, w5, w6, w7), np.uint8)
    r[32:32 + cap] = payload[:cap]
    return r


def kat_events(sc, cases, want, wantf, model):
    """The ring the KAT batch must leave with GF_NETDEV_F_TRACE_NOTIFY, per packet in the order the
    programs send: from_netdev's TRACE_FROM_HOST / FROM_PROXY (bpf_netdev.c:423-433; ifindex =
    ingress_ifindex, the frame as received), encap_and_redirect's TRACE_TO_OVERLAY (encap.h:67: the
    secctx, ENCAP_IFINDEX, the frame as rewritten), then the drop notification: handle_policy's
    (src_label, SECLABEL, LXC_ID, ifindex; drop.h:47-107) or the caller's send_drop_notify_error
    (zeros).  No KAT endpoint has TRACE_NOTIFY, so there is no TRACE_TO_LXC."""
    pk = sc.batches[0]
    eps = {e["lxc_id"]: e for e in sc.lxc}
    ifx = {ep["lxc_id"]: ep["ifindex"] for ep in model.eps.values()}
    out = []
    for i, c in enumerate(cases):
        ln, o = int(pk.lens[i]), want[i]
        obs, src = HM.trace_first(c["mark"])
        out.append(_event(4 | (obs << 8), ln, src, 0, 0, sc.host["ingress_ifindex"], pk.frames[i]))
        if o["stage"] == 7 and o["action"] == 7 and not o["flags"] & 0x20:
            out.append(_event(4 | (4 << 8), ln, int(model.secctx[i]), 0, 0, sc.node["encap_ifindex"], wantf[i]))
        if o["action"] == 2:
            e = eps.get(int(o["lxc_id"])) if o["stage"] == 4 else None
            if e is None:
                out.append(_event(1 | (int(o["reason"]) << 8), ln, 0, 0, 0, 0, wantf[i]))
            else:
                out.append(_event(1 | (int(o["reason"]) << 8) | (e["lxc_id"] << 16), ln, int(model.secctx[i]) & 0xffff,
                                  e["seclabel"], e["lxc_id"], ifx[e["lxc_id"]], wantf[i]))
    return np.stack(out)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["A", "B"])
def test_gpu_kat_events(variant):
    """The event ring over the marked KAT batches with GF_NETDEV_F_TRACE_NOTIFY: each packet's first
    record is TRACE_FROM_PROXY with the proxy's identity (marks 0xFEA / 0xFEB with one) or
    TRACE_FROM_HOST with HOST_ID (mark 0, 0x00000FEA, a near-miss magic), the encap hits add
    TRACE_TO_OVERLAY with the packet's secctx and ENCAP_IFINDEX, the drops their notification."""
    _gpu()
    import ctypes as C
    from cilium_amd._lib import lib, gf_event_ring
    from cilium_amd.datapath import Datapath
    sc, cases, want, wantf = kat_scenario(variant)
    sc.host["flags"] |= synth.NETDEV_TRACE_NOTIFY
    model = HM.HostModel(sc)
    got_m, _, _, _ = model_run(sc, sc.batches[0], sc.now, OracleDP(sc), model)
    assert (got_m == want).all()
    exp = kat_events(sc, cases, want, wantf, model)
    sub = set(exp[exp[:, 0] == 4][:, 1].tolist())
    assert {6, 7} <= sub and (variant == "A" or 4 in sub) and (exp[:, 0] == 1).sum() >= 1
    recs = torch.zeros((1024, 160), dtype=torch.uint8, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
    ring = gf_event_ring(recs.data_ptr(), 1024, cnt.data_ptr())
    dp = Datapath(sc, pin_prefix=None)
    assert lib.gf_set_event_ring(C.byref(ring)) == 0
    try:
        got, snap = _gpu_host(dp, sc.batches[0], sc.now)
        _same(got, want, "records")
        assert not (snap != wantf).any()
        n = int(cnt.item())
        g = recs[:n].cpu().numpy()
        assert n == len(exp), (n, len(exp))
        bad = np.nonzero((g != exp).any(axis=1))[0]
        assert len(bad) == 0, f"{len(bad)} event records differ, first {bad[:1]}: {g[bad[0]][:40]} vs {exp[bad[0]][:40]}"
    finally:
        lib.gf_set_event_ring(None)
        dp.close()


@pytest.mark.gpu
@pytest.mark.parametrize("seed,events", [(3, False), (8, False), (3, True)])
def test_gpu_coincidence(seed, events):
    """gf_host_classify against OracleDP.pipeline and gf_pipeline_classify on the coincidence
    batches: records, frames (bytes 0-5 of the packets that end after rewrite_dmac_to_host are
    CILIUM_NET_MAC), every CT / policy / proxy map; with the event ring the ring against the
    oracle's, where only each packet's first record differs: subtype 8 -> 7, src_label 0 ->
    HOST_ID."""
    _gpu()
    import ctypes as C
    from cilium_amd._lib import lib, gf_event_ring
    from cilium_amd.datapath import Datapath, DeviceBatch, to_numpy
    sc, nd = coincidence_scenario(seed, trace=events)
    if events:
        cap = 200000
        recs = torch.zeros((cap, 160), dtype=torch.uint8, device="cuda")
        cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
        ring = gf_event_ring(recs.data_ptr(), cap, cnt.data_ptr())
    try:
        dp, pipe = Datapath(sc, pin_prefix=None), OracleDP(nd)
        if events:
            assert lib.gf_set_event_ring(C.byref(ring)) == 0
        exp, kept = [], []
        for bi, pk in enumerate(sc.batches):
            got, snap = _gpu_host(dp, pk, sc.now + bi)
            with O.TraceSink(pk.n) as ts:
                ro, _, rs = pipe.pipeline(pk, sc.now + bi)
            want = renamed(ro)
            _same(got, want, f"b{bi}")
            rs, dm = _coincidence_frames(pk, want, rs)
            assert dm.any() and not (snap != rs).any(), f"frames b{bi}"
            kept.append((got, snap, dm))
            exp.append(ts.events())
        names = ["ct4", "ct6", "cilium_proxy4", "cilium_proxy6"] + [e["policy"] for e in sc.lxc]
        dumps = {name: dp.dump_map(name) for name in names}
        for name in names:
            assert dumps[name] == pipe.dump(name), name
        dp.close()
        if not events:                                  # gf_pipeline_classify itself (the node config is one per
            dpn = Datapath(nd, pin_prefix=None)         # process, so it runs after the from-host datapath is closed)
            for bi, pk in enumerate(sc.batches):
                got, snap, dm = kept[bi]
                po, _, psnap = dpn.pipeline(DeviceBatch(pk, parse=False), sc.now + bi)
                torch.cuda.synchronize()
                _same(got, renamed(to_numpy(po, PIPE_OUT)), f"pipeline b{bi}")
                ps = psnap.cpu().numpy()
                ps[dm, 0:6] = np.frombuffer(NET_MAC, np.uint8)
                assert not (snap != ps).any(), f"pipeline frames b{bi}"
            for name in names:
                assert dumps[name] == dpn.dump_map(name), name
            dpn.close()
        if events:
            e = np.concatenate(exp)
            tr = (e[:, 0] == 4) & (e[:, 1] == 8)
            e[tr, 1] = 7                                # TRACE_FROM_STACK -> TRACE_FROM_HOST
            e[tr, 16:20] = np.frombuffer(struct.pack("<I", HM.HOST_ID), np.uint8)   # src_label
            # a drop record captures the frame as it is dropped: with CILIUM_NET_MAC where the program
            # ended after rewrite_dmac_to_host (every packet's records begin with its trace record)
            owner = np.cumsum(tr) - 1
            dmall = np.concatenate([k[2] for k in kept])
            drop = (e[:, 0] == 1) & dmall[owner]
            assert drop.any()
            e[drop, 32:38] = np.frombuffer(NET_MAC, np.uint8)
            n = int(cnt.item())
            assert n == len(e) and tr.sum() == sum(pk.n for pk in sc.batches) and (e[:, 0] == 1).sum() > 100
            g = recs[:n].cpu().numpy()
            bad = np.nonzero((g != e).any(axis=1))[0]
            assert len(bad) == 0, f"{len(bad)} event records differ, first {bad[:1]}: {g[bad[0]][:32]} vs {e[bad[0]][:32]}"
    finally:
        if events:
            lib.gf_set_event_ring(None)


@pytest.mark.gpu
@pytest.mark.parametrize("seed,kind", FUZZ)
def test_gpu_host_fuzz(seed, kind):
    """host_fuzz (marks, reverse hits, encap, host and local destinations) against the model +
    OracleDP.ingress: records, frames, ct4 / ct6 (and the per-endpoint CT maps), every policy
    map, cilium_proxy4 / 6 — plain, with ConntrackLocal and with Conntrack off on every 2nd
    endpoint (tests/ctoff_model.py for those)."""
    _gpu()
    from cilium_amd.datapath import Datapath
    sc, off = fuzz_scenario(seed, kind)
    dp, ref, model = Datapath(sc, pin_prefix=None), OracleDP(sc), HM.HostModel(sc)
    ctoff = CM.CtOffModel(sc) if off else None
    for bi, pk in enumerate(sc.batches):
        got, snap = _gpu_host(dp, pk, sc.now + bi)
        want, frames, _, _ = model_run(sc, pk, sc.now + bi, ref, model, ctoff, off)
        _same(got, want, f"b{bi}")
        cmp = _frames_cmp(pk, want)
        assert (want["stage"][~cmp] == 4).all()
        _frames_same(snap, frames, cmp, want, f"frames b{bi}")
    ct = sorted({e[k] for e in sc.lxc for k in ("ct4", "ct6") if e.get(k)})
    for name in ct + ["cilium_proxy4", "cilium_proxy6"]:
        assert dp.dump_map(name) == ref.dump(name), name
    for e in sc.lxc:
        want = ctoff.progs[e["lxc_id"]].policy_dump() if e["lxc_id"] in off else ref.dump(e["policy"])
        assert dp.dump_map(e["policy"]) == want, e["policy"]
    if off:
        assert not ctoff.proxy4 and not ctoff.proxy6
    dp.close()


def _csum16(x):
    if len(x) & 1:
        x += b"\0"
    t = sum(struct.unpack(">%dH" % (len(x) // 2), x))
    while t >> 16:
        t = (t & 0xffff) + (t >> 16)
    return ~t & 0xffff


def _reply(v6, src, dst, nh, sport_raw, dport_raw):
    """A frame from the proxy, built field by field with whole-frame checksums."""
    if nh == 6:
        l4 = sport_raw + dport_raw + struct.pack(">IIBBHHH", 7, 9, 0x50, 0x12, 512, 0, 0)
    else:
        l4 = sport_raw + dport_raw + struct.pack(">HH", 12, 0) + b"pong"
    co = 16 if nh == 6 else 6
    ph = src + dst + (struct.pack(">IHBB", len(l4), 0, 0, nh) if v6 else struct.pack(">BBH", 0, nh, len(l4)))
    l4 = l4[:co] + struct.pack(">H", _csum16(ph + l4) or 0xffff) + l4[co + 2:]
    eth = bytes.fromhex("020202020202040404040404")
    if v6:
        return eth + b"\x86\xdd" + struct.pack(">IHBB", 0x60000000, len(l4), nh, 64) + src + dst + l4
    h = struct.pack(">BBHHHBBH", 0x45, 0, 20 + len(l4), 1, 0, 64, nh, 0) + src + dst
    return eth + b"\x08\x00" + h[:10] + struct.pack(">H", _csum16(h)) + h[12:] + l4


@pytest.mark.gpu
def test_gpu_round_trip():
    """What the entry point is for, all on the device.  A pipeline batch whose clients are local
    endpoints hits L7 rules and writes cilium_proxy4 / 6.  The proxy's replies — source the
    proxy's address and port, destination the client, mark 0xFEB | identity << 16 — go through
    gf_host_classify and must come out with the original server address and port as source,
    checksums that a full recomputation accepts, the skip-proxy bit in effect (no second
    redirect), delivered to the client's endpoint with the model's handle_policy verdict, and
    the proxy maps unchanged by the call."""
    _gpu()
    from cilium_amd.datapath import Datapath, DeviceBatch, to_numpy
    sc = synth.pipeline_fuzz(seed=11, n_packets=6000, n_batches=1)
    sc.host = dict(sc.netdev, ingress_ifindex=5, cilium_net_mac=NET_MAC)
    lxc = sc.maps["cilium_lxc"]
    ep4 = {bytes(k[:4]): int(v[6]) | (int(v[7]) << 8) for k, v in zip(lxc.keys, lxc.vals) if k[16] == 1 and not v[8] & 1}
    ep6 = {bytes(k[:16]): int(v[6]) | (int(v[7]) << 8) for k, v in zip(lxc.keys, lxc.vals) if k[16] == 2 and not v[8] & 1}
    pk = sc.batches[0]
    # clients without a port map: pipeline_fuzz's duplicated portmap entries each correct the checksum
    # from the old port (l4.h:84-88), which by the reference's own rule leaves it wrong
    plain = {bytes(k[:16]) for k, v in zip(lxc.keys, lxc.vals) if not v[48:52].any()}
    l4a = sorted(a for a in ep4 if a + bytes(12) in plain)
    l6a = sorted(a for a in ep6 if a in plain)
    assert len(l4a) > 3 and len(l6a) > 3
    for i in range(pk.n):                               # every client is a local endpoint
        if pk.frames[i, 12] == 0x08:
            pk.frames[i, 26:30] = np.frombuffer(l4a[i % len(l4a)], np.uint8)
        elif pk.frames[i, 12] == 0x86:
            pk.frames[i, 22:38] = np.frombuffer(l6a[i % len(l6a)], np.uint8)
    dp, ref, model = Datapath(sc, pin_prefix=None), OracleDP(sc), HM.HostModel(sc)
    po, _, _ = dp.pipeline(DeviceBatch(pk, parse=False), sc.now)
    torch.cuda.synchronize()
    po = to_numpy(po, PIPE_OUT)
    ro, _, _ = ref.pipeline(pk, sc.now)
    _same(po, ro, "pipeline")
    assert ((po["stage"] == 4) & (po["flags"] & 1 != 0) & (po["action"] == 7)).sum() > 50
    d4, d6 = dp.dump_map("cilium_proxy4"), dp.dump_map("cilium_proxy6")
    assert d4 == ref.dump("cilium_proxy4") and d6 == ref.dump("cilium_proxy6") and len(d4) > 10 and len(d6) > 4
    nd = sc.node
    gw, host6 = struct.pack("<I", nd["ipv4_gateway"]), bytes(nd["host_ip6"])
    frames, lens, mark, expect = [], [], [], []
    for v6, d, alen, proxy in ((False, d4, 4, gw), (True, d6, 16, host6)):
        for key, val in sorted(d.items()):              # one reply per entry the redirects wrote
            client, pport, cport, nh = key[:alen], key[alen:alen + 2], key[alen + 2:alen + 4], key[alen + 4]
            fr = _reply(v6, proxy, client, nh, pport, cport)
            row = np.zeros(128, np.uint8)
            row[:len(fr)] = np.frombuffer(fr, np.uint8)
            frames.append(row)
            lens.append(len(fr))
            mark.append(0xFEB | ((struct.unpack_from("<I", val, alen + 4)[0] & 0xffff) << 16))
            expect.append((v6, val[:alen], val[alen:alen + 2], (ep6 if v6 else ep4)[client]))
    n = len(frames)
    rp = Packets(np.stack(frames), np.array(lens, np.uint32), None, None, None, np.zeros(n, np.uint8),
                 np.zeros(n, np.uint32), None, np.array(mark, np.uint32))
    got, snap = _gpu_host(dp, rp, sc.now + 1)
    want, wframes, _, (dl, sub) = model_run(sc, rp, sc.now + 1, ref, model)
    _same(got, want, "replies")
    assert len(dl) == n and (sub.tc_index & 1).all()
    seen = set()
    for i, (v6, saddr, sport, lxc_id) in enumerate(expect):
        a0, l4 = (22, 54) if v6 else (26, 34)
        assert bytes(snap[i, a0:a0 + len(saddr)]) == saddr and bytes(snap[i, l4:l4 + 2]) == sport, i
        assert _valid_checksums(snap[i], lens[i]), i
        assert got["stage"][i] == 4 and got["flags"][i] & 0x10 and not got["flags"][i] & 1 and got["lxc_id"][i] == lxc_id, i
        seen.add((v6, int(snap[i, 20 if v6 else 23])))
    assert {(False, 6), (True, 6)} <= seen and (got["action"] == 7).any()
    cmp = _frames_cmp(rp, want)
    assert not (snap[cmp] != wframes[cmp]).any()
    assert dp.dump_map("cilium_proxy4") == d4 and dp.dump_map("cilium_proxy6") == d6
    dp.close()


_EDGE = {}


def _edge_case():
    """One seed: 257 host_fuzz packets whose every touched header byte lies in the first 64
    bytes, so that the same packets can be cut to every stride."""
    if not _EDGE:
        sc, _ = fuzz_scenario(6, "plain", n_packets=3000, n_batches=1)
        pk = sc.batches[0]
        cols = OracleDP(sc).parse(pk)
        need = np.where(cols["proto"] == 6, 18, np.where(np.isin(cols["proto"], (17, 1, 58)), 8, 4))
        ip = np.isin(cols["ethertype"], (0x0800, 0x86DD))
        ok = ~ip | ((cols["l4_off"] >= 34) & (cols["l4_off"] + need <= 64))
        _EDGE["sc"], _EDGE["pk"] = sc, _subset(pk, np.nonzero(ok)[0][:257])
        assert _EDGE["pk"].n == 257
    return _EDGE["sc"], _EDGE["pk"]


@pytest.mark.gpu
@pytest.mark.parametrize("stride", [64, 70, 128, 144, 256])
def test_gpu_tile_and_copy_edges(stride):
    """n around the 64-lane wave and the 128- and 256-lane tiles x strides on the uint4 path
    (64, 128), the byte path (70) and the 128-lane tile (144, 256), with and without snap_out,
    and with mark, tc_index and flow_hash present or NULL, against the model: the calls run one
    after the other on one datapath and one oracle, each the first n packets of one batch."""
    _gpu()
    from cilium_amd.datapath import Datapath
    sc, full = _edge_case()
    dp, ref, model = Datapath(sc, pin_prefix=None), OracleDP(sc), HM.HostModel(sc)
    for n in (1, 63, 64, 65, 127, 128, 129, 257):
        for snap_out, bare in ((True, False), (False, True), (True, True)):
            pk = full.slice(0, n)
            pk = Packets(np.ascontiguousarray(pk.frames[:, :stride]), pk.lens, None, None, None,
                         None if bare else pk.tc_index, None if bare else pk.flow_hash, None, None if bare else pk.mark)
            got, snap = _gpu_host(dp, pk, sc.now, snap_out=snap_out, bare=bare)
            want, frames, _, _ = model_run(sc, pk, sc.now, ref, model)
            _same(got, want, f"n {n} stride {stride} snap_out {snap_out} bare {bare}")
            if snap_out:
                cmp = _frames_cmp(pk, want)
                assert not (snap[cmp] != frames[cmp]).any(), (n, stride)
    dp.close()


@pytest.mark.gpu
def test_gpu_refusals():
    _gpu()
    import ctypes as C
    from cilium_amd._lib import lib, gf_frames, gf_host_batch
    from cilium_amd.datapath import Datapath, DeviceBatch
    sc, cases, want, wantf = kat_scenario("A")
    dp = Datapath(sc, pin_prefix=None)
    b = DeviceBatch(sc.batches[0], parse=False)
    out = torch.empty((b.n, 24), dtype=torch.uint8, device="cuda")

    def call(host, n, stride, frames=b.frames.data_ptr(), lens=b.len.data_ptr(), o=out.data_ptr()):
        hb = gf_host_batch(gf_frames(n, stride, frames, lens), b.mark.data_ptr(), None, None)
        return lib.gf_host_classify(host, C.byref(hb), sc.now, o, None, None)

    assert call(dp.host, 0, 128) == 0
    assert call(dp.host, b.n, 13) == -errno.EINVAL
    assert call(dp.host, b.n, 272) == -errno.EINVAL
    assert call(dp.host, b.n, 128, frames=None) == -errno.EFAULT
    assert call(dp.host, b.n, 128, lens=None) == -errno.EFAULT
    assert call(dp.host, b.n, 128, o=None) == -errno.EFAULT
    assert call(dp.pipe or 987654, b.n, 128) == -errno.EBADF
    assert lib.gf_host_classify(dp.host, None, sc.now, out.data_ptr(), None, None) == -errno.EFAULT
    torch.cuda.synchronize()
    dp.close()
