"""The pipeline's netdev stage as bpf/init.sh builds the native device's object: GF_NETDEV_F_HANDLE_NS
(icmp6_handle's NS / echo-to-router tail calls) and GF_NETDEV_F_ENCAP (encap_and_redirect for pods of
other nodes), through gf_pipeline_classify_tunnel.

The CPU oracle's from_netdev has neither option.  The checks rest on:

 1. hand-derived known answers (tests/golden/netdev_kats.json; expected checksums are whole-frame
    recomputations);
 2. options off: the pipeline is today's, bit for bit, against OracleDP.pipeline;
 3. gf_host_classify, whose encap branch is tested on its own (tests/test_from_host.py): with no XDP /
    LB program, marks 0 and empty proxy maps the two programs differ by rewrite_dmac_to_host alone;
 4. tests/netdev_model.py, a per-frame restatement of from_netdev with the two options, behind the
    oracle's bpf_xdp / bpf_lb and in front of OracleDP.ingress (or tests/ctoff_model.py);
 5. tests/respond_model.py for the replies gf_respond builds from the pipeline's records.

Frames against the model: handle_policy writes frames and OracleDP.ingress returns none, so the frames
of the packets the front ends (always, in full) and of IPv4 deliveries forwarded as CT_NEW /
CT_ESTABLISHED without a proxy redirect are compared (as tests/test_from_host.py).
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
from tests import netdev_model as NM
from tests.overlay_model import PIPE_OUT

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KAT_NOW = 5000
OPTS = synth.NETDEV_HANDLE_NS | synth.NETDEV_ENCAP
KAT_NAMES = {"ns_router", "ns_other_target", "ns_behind_hopbyhop", "echo_router", "echo_pod", "udp_first_byte_135",
             "icmp6_len54", "encap_v4_hit", "encap_v6_hit", "encap_v4_tunnel_miss", "encap_v6_tunnel_miss",
             "outside_cluster", "local_endpoint", "host_endpoint", "lb_remote_backend"}
ROUTER = bytes.fromhex("20010db8aabb" + "00" * 10)


def _subset(pk, m):
    f = lambda x: None if x is None else x[m]
    return Packets(pk.frames[m], pk.lens[m], f(pk.src_identity), f(pk.ifindex), f(pk.lxc_id), f(pk.tc_index),
                   f(pk.flow_hash))


# ---------------------------------------------------------------- KATs
def _kats():
    with open(os.path.join(GOLDEN, "netdev_kats.json")) as f:
        return json.load(f)["cases"]


def kat_scenario(variant, flags=OPTS):
    """The KATs of one variant as one batch (A: the tunnel map holds 10.77.2.0 and ROUTER_IP/96; B:
    10.77.2.0 alone).  No XDP program; bpf_lb with the service 10.96.0.1:80 -> 10.77.2.5:8080.
    Returns (scenario, cases, expected records, expected frames, expected tunnel_ip)."""
    cases = [c for c in _kats() if c["variant"] == variant]
    sc = synth.Scenario(f"netdev_kats{variant}", now=KAT_NOW, host_ifindex=3)
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
    sc.add_map(synth.MapSpec("cilium_lxc", synth.HASH, 20, 112, 1024, 0, keys, vals))
    sc.add_map(synth.MapSpec("ct4", synth.LRU_HASH, 14, 48, 4096, 0))
    sc.add_map(synth.MapSpec("ct6", synth.LRU_HASH, 40, 48, 4096, 0))
    for k, lid in enumerate((3000, 3001)):
        sc.add_map(synth.MapSpec(f"pol{k}", synth.HASH, 8, 24, 1024, 0, synth.policy_keys([300], [0], [0]),
                                 synth.policy_vals([0])))
        sc.lxc.append({"lxc_id": lid, "seclabel": 500 + k, "policy": f"pol{k}", "ct4": "ct4", "ct6": "ct6",
                       "flags": synth.LXC_PRODUCTION, "l4": []})
    vip, be = [synth.ip4("10.96.0.1")] * 2, [0, synth.ip4("10.77.2.5")]
    sc.add_map(synth.MapSpec("lb4_svc", synth.HASH, 8, 12, 64, 0, synth.lb4_keys(vip, [80, 80], [0, 1]),
                             synth.lb4_vals(be, [0, 8080], [1, 0], [7, 7])))
    sc.lb = {"lb4": "lb4_svc", "flags": synth.LB_L3 | synth.LB_L4}
    sc.add_map(synth.MapSpec("cilium_proxy4", synth.HASH, 10, 16, 1024, 0))
    sc.add_map(synth.MapSpec("cilium_proxy6", synth.HASH, 22, 28, 1024, 0))
    tk = [synth.endpoint_keys4([synth.ip4("10.77.2.0")])]
    if variant == "A":
        tk.append(synth.endpoint_keys6(np.frombuffer(ROUTER, np.uint8)[None, :]))
    tk = np.concatenate(tk)
    tv = synth.endpoint_keys4([synth.ip4("192.168.9.1"), synth.ip4("192.168.9.2")][:len(tk)])
    sc.add_map(synth.MapSpec("cilium_tunnel_map", synth.HASH, 20, 20, 64, 0, tk, tv))
    sc.node = {"proxy4": "cilium_proxy4", "proxy6": "cilium_proxy6", "host_mac": bytes.fromhex("ce72a7038856"),
               "node_mac": bytes.fromhex("deadbeefc0de"), "ipv4_gateway": 0xfffff50a, "encap_ifindex": 9,
               "tunnel_map": "cilium_tunnel_map", "router_ip6": ROUTER, "ipv4_cluster_range": 0x00004d0a,
               "ipv4_cluster_mask": 0x0000ffff, "ipv4_mask": 0x00ffffff}
    sc.netdev = {"lxc_map": "cilium_lxc", "flags": flags, "fixed_secctx": 0, "router_ip6": ROUTER, "ingress_ifindex": 4}
    n, S = len(cases), 128
    frames, lens = np.zeros((n, S), np.uint8), np.zeros(n, np.uint32)
    want, wantf, wtun = np.zeros(n, PIPE_OUT), np.zeros((n, S), np.uint8), np.zeros(n, np.uint32)
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
        wtun[k] = c["tunnel_ip"]
    sc.batches.append(Packets(frames, lens, None, None, None, np.zeros(n, np.uint8), np.zeros(n, np.uint32)))
    return sc, cases, want, wantf, wtun


def model_run(sc, pk, now, ref, pre, model, ctoff=None, off=()):
    """bpf_xdp / bpf_lb by `pre`, the model's from_netdev, then handle_policy of the delivered subset in
    batch order: the oracle's, or tests/ctoff_model.py for endpoints without conntrack.  Returns
    (records, new_daddr6, front frames, tunnel_ip, front records, (delivered indices, subset))."""
    rec, nd6, frames, tun, dl, sub = model.front(pk, pre, now)
    ing = np.zeros(sub.n, CM.ING_OUT)
    if sub.n:
        offm = np.isin(sub.lxc_id, list(off)) if ctoff is not None else np.zeros(sub.n, bool)
        if (~offm).any():
            s2 = Packets(sub.frames[~offm], sub.lens[~offm], sub.src_identity[~offm], sub.ifindex[~offm],
                         sub.lxc_id[~offm], None if sub.tc_index is None else sub.tc_index[~offm],
                         None if sub.flow_hash is None else sub.flow_hash[~offm])
            ing[~offm] = ref.ingress(s2, now)
        if offm.any():
            idx, mrec, _ = ctoff.batch(sub, ref.parse(sub), now, mask=offm)
            assert np.array_equal(idx, np.nonzero(offm)[0])
            ing[offm] = mrec
    return NM.complete(rec, dl, ing), nd6, frames, tun, rec, (dl, sub)


def test_kats_cover_the_issue_list():
    names = [c["name"] for c in _kats()]
    assert len(names) == len(set(names)) and set(names) == KAT_NAMES and all(c["derivation"] for c in _kats())


@pytest.mark.parametrize("variant", ["A", "B"])
def test_model_reproduces_every_kat(variant):
    sc, cases, want, wantf, wtun = kat_scenario(variant)
    got, _, frames, tun, _, _ = model_run(sc, sc.batches[0], sc.now, OracleDP(sc), NM.pre_oracle(sc), NM.NetdevModel(sc))
    for k, c in enumerate(cases):
        assert got[k] == want[k], (c["name"], got[k], want[k])
        assert bytes(frames[k]) == bytes(wantf[k]), c["name"]
        assert tun[k] == wtun[k], c["name"]


def test_kat_frames_without_the_options_are_todays():
    """What the KATs pin: without the flags the oracle's from_netdev sends the responder frames on (the
    echo to the router and the NS end as TC_ACT_OK or in a delivery) and passes every remote-pod
    destination to the stack, although gf_node_cfg.encap_ifindex is set."""
    sc, cases, want, wantf, wtun = kat_scenario("A", flags=0)
    ro, _, rs = OracleDP(sc).pipeline(sc.batches[0], sc.now)
    got, _, frames, tun, _, _ = model_run(sc, sc.batches[0], sc.now, OracleDP(sc), NM.pre_oracle(sc), NM.NetdevModel(sc))
    assert (got == ro).all() and not tun.any() and not (ro["flags"] & 0x0c).any() and not ro["pad0"].any()
    by = {c["name"]: ro[k] for k, c in enumerate(cases)}
    assert by["encap_v4_hit"]["action"] == 0 and by["lb_remote_backend"]["action"] == 0 and by["ns_router"]["action"] == 0
    assert by["lb_remote_backend"]["daddr4"] == 0x05024d0a


# ---------------------------------------------------------------- the tie to the oracle
def test_model_against_oracle_without_options():
    """On a batch that triggers neither option (flags 0) the model — the oracle's bpf_xdp / bpf_lb, the
    restated from_netdev, OracleDP.ingress — equals OracleDP.pipeline: records, new_daddr6, frames, maps."""
    sc = synth.pipeline_fuzz(seed=3, n_packets=4000, n_batches=2)
    ref, pipe, pre, model = OracleDP(sc), OracleDP(sc), NM.pre_oracle(sc), NM.NetdevModel(sc)
    seen = set()
    for bi, pk in enumerate(sc.batches):
        got, nd6, frames, tun, _, _ = model_run(sc, pk, sc.now + bi, ref, pre, model)
        ro, rn6, rs = pipe.pipeline(pk, sc.now + bi)
        bad = np.nonzero(got != ro)[0]
        assert len(bad) == 0, f"b{bi}: {len(bad)} differ, first {bad[:1]}: {got[bad[:1]]} != {ro[bad[:1]]}"
        assert np.array_equal(nd6, rn6) and not tun.any() and not model.opt.any()
        cmp = _frames_cmp(pk, ro)
        assert cmp.sum() > pk.n // 3 and not (frames[cmp] != rs[cmp]).any(), f"frames b{bi}"
        seen |= set(zip(ro["stage"].tolist(), ro["action"].tolist()))
    for name in ["ct4", "ct6", "cilium_proxy4", "cilium_proxy6"] + [e["policy"] for e in sc.lxc]:
        assert ref.dump(name) == pipe.dump(name), name
    assert {(1, 1), (2, 2), (3, 0), (3, 2), (3, 7), (4, 2), (4, 7)} <= seen, seen   # handle_policy forwards by redirect


def _frames_cmp(pk, want):
    """Packets whose frame handle_policy does not write (see the module docstring)."""
    return (want["stage"] != 4) | ((pk.frames[:, 12] == 0x08) & (want["flags"] & 1 == 0) & (want["action"] != 2) &
                                   (want["ct_ret"] < 2))


# ---------------------------------------------------------------- netdev_fuzz
def fuzz_scenario(seed, kind, n_packets=4000, n_batches=1, stride=256, trace=False):
    sc = synth.netdev_fuzz(seed=seed, n_packets=n_packets, n_batches=n_batches)
    off = []
    if kind == "ctoff":
        off = synth.conntrack_off(sc, every=2)
        for e in sc.lxc:                                # cilium_proxy4 / 6 are shared with the CT-on half
            if e["lxc_id"] in off:
                sc.maps[e["policy"]].vals[:, 0:2] = 0
    if trace:
        for k, e in enumerate(sc.lxc):
            if k % 3 == 0:
                e["flags"] |= synth.LXC_TRACE_NOTIFY
        sc.netdev = dict(sc.netdev, flags=sc.netdev["flags"] | synth.NETDEV_TRACE_NOTIFY)
    if stride != 256:
        for bi, pk in enumerate(sc.batches):
            sc.batches[bi] = Packets(np.ascontiguousarray(pk.frames[:, :stride]), pk.lens, pk.src_identity, pk.ifindex,
                                     pk.lxc_id, pk.tc_index, pk.flow_hash)
    return sc, off


def test_synth_generators_unchanged_by_the_new_helper():
    """netdev_fuzz is a new helper over host_fuzz: the existing generators produce the bytes they did."""
    import hashlib
    a, b = synth.pipeline_fuzz(seed=3, n_packets=600, n_batches=1), synth.pipeline_fuzz(seed=3, n_packets=600, n_batches=1)
    synth.netdev_fuzz(seed=3, n_packets=600, n_batches=1)
    c = synth.pipeline_fuzz(seed=3, n_packets=600, n_batches=1)
    h = lambda s: hashlib.sha256(s.batches[0].frames.tobytes() + s.batches[0].lens.tobytes()).hexdigest()
    assert h(a) == h(b) == h(c) and a.netdev["flags"] == 0


@pytest.mark.parametrize("kind", ["plain", "ctoff"])
def test_netdev_fuzz_is_not_thin(kind):
    """The batch the GPU fuzz cases use shows, by the model and the reference alone: both tail calls,
    an NS behind a hop-by-hop header that is not answered, a type byte that cannot be loaded, v4 and v6
    encap redirects, a tunnel miss, an LB-translated frame, deliveries with allows and denies, CT
    entries created, a drop at the front, an ICMP6_TE, an LB verdict, and no class above 60 %."""
    sc, off = fuzz_scenario(3, kind)
    ref, pre, model = OracleDP(sc), NM.pre_oracle(sc), NM.NetdevModel(sc)
    ctoff = CM.CtOffModel(sc) if off else None
    pk = sc.batches[0]
    got, _, frames, tun, _, (dl, sub) = model_run(sc, pk, sc.now, ref, pre, model, ctoff, off)
    s3, s4 = got["stage"] == 3, got["stage"] == 4
    resp, enc = s3 & (got["flags"] & 4 != 0), s3 & (got["flags"] & 8 != 0)
    v4, v6 = pk.frames[:, 12] == 0x08, pk.frames[:, 12] == 0x86
    assert (resp & (got["pad0"] == 2)).any() and (resp & (got["pad0"] == 3)).any()
    assert not (got["pad0"][~resp]).any() and (tun != 0).tolist() == enc.tolist()
    hbh = v6 & (pk.frames[:, 20] == 0) & (pk.frames[:, 54] == 58) & (pk.frames[:, 62] == 135)
    assert hbh.any() and not (hbh & resp).any()
    short = v6 & (pk.frames[:, 20] == 58) & (pk.lens == 54)
    assert (short & s3 & (got["action"] == 0) & model.opt).any()
    assert (enc & v4).any() and (enc & v6).any() and (got["action"][enc] == 7).all() and (got["ifindex_lo"][enc] == 7).all()
    in_cluster = v4 & (pk.lens >= 34) & (model.post_lb[:, 30] == 10) & (model.post_lb[:, 31] == 77)
    assert (in_cluster & s3 & (got["action"] == 0)).any(), "tunnel miss"
    assert (got["flags"] & 0x40 != 0).any() and (got["stage"] == 2).any()
    assert (s4 & (got["action"] != 2)).any() and (s4 & (got["reason"] == 133)).any()
    assert (s4 & (got["flags"] & 2 != 0)).any(), "CT created"
    assert (s3 & (got["action"] == 2)).any() and (s3 & (got["flags"] & 0x20 != 0)).any()
    for name, m in {"delivered": s4, "encap": enc, "responder": resp, "stack": s3 & (got["action"] == 0)}.items():
        assert m.sum() * 10 <= pk.n * 6, (name, int(m.sum()), pk.n)
    assert resp.sum() * 100 >= pk.n and enc.sum() * 100 >= 2 * pk.n


# ---------------------------------------------------------------- error returns without a device
def test_pipeline_load_encap_needs_the_node():
    import ctypes as C
    from cilium_amd import bpf
    from cilium_amd._lib import lib, gf_netdev_cfg, gf_node_cfg, gf_pipeline_cfg
    lxc = bpf.CreateMap(synth.HASH, 20, 112, 64, 0)
    tun = bpf.CreateMap(synth.HASH, 20, 20, 64, 0)
    arr = lib.gf_policy_array_create()
    z16, z6 = (C.c_uint8 * 16)(), (C.c_uint8 * 6)()
    node = lambda ifx, t: gf_node_cfg(1, 0, 0, 0, z16, z6, z6, 0, 0, 0, 0, 0, ifx, t, z16)
    cfg = lambda fl: gf_pipeline_cfg(0, 0, gf_netdev_cfg(lxc, fl, 0, z16, 4), arr)
    try:
        for ifx, t, fl, ok in ((0, tun, synth.NETDEV_ENCAP, False), (9, 0, synth.NETDEV_ENCAP, False),
                               (9, tun, synth.NETDEV_ENCAP, True), (0, 0, synth.NETDEV_HANDLE_NS, True),
                               (9, tun, 0, True), (0, 0, 0, True)):
            assert lib.gf_node_config(C.byref(node(ifx, t))) == 0
            h = lib.gf_pipeline_load(C.byref(cfg(fl)))
            assert (h > 0) if ok else (h == -errno.EINVAL), (ifx, t, fl, h)
            if h > 0:
                bpf.ObjClose(h)
    finally:
        lib.gf_node_config(C.byref(node(0, 0)))
        for h in (arr, lxc, tun):
            bpf.ObjClose(h)


# ---------------------------------------------------------------- GPU
torch = pytest.importorskip("torch")


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(0)


def _gpu_pipe(dp, pk, now, snap_out=True, tunnel_ip=True, bare=False):
    from cilium_amd.datapath import DeviceBatch, to_numpy
    b = DeviceBatch(pk, parse=False)
    if bare:
        b.tc_index = b.flow_hash = None
    out, nd6, snap, tun = dp.pipeline_tunnel(b, now, snap_out=snap_out, tunnel_ip=tunnel_ip)
    torch.cuda.synchronize()
    return (to_numpy(out, PIPE_OUT), nd6.cpu().numpy(), None if snap is None else snap.cpu().numpy(),
            None if tun is None else tun.cpu().numpy().view(np.uint32))


def _same(got, want, what):
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, f"{what}: {len(bad)} records differ, first {bad[:1]}: {got[bad[:1]]} != {want[bad[:1]]}"


def _frames_same(snap, frames, cmp, want, what):
    bad = np.nonzero(cmp & (snap != frames).any(axis=1))[0]
    if len(bad):
        i = bad[0]
        off = np.nonzero(snap[i] != frames[i])[0]
        raise AssertionError(f"{what}: {len(bad)} frames differ, first {i} {want[i]} at offsets {off[:12]}: "
                             f"{bytes(snap[i][off[:12]]).hex()} != {bytes(frames[i][off[:12]]).hex()}")


def _ring(cap=200000):
    from cilium_amd._lib import gf_event_ring
    recs = torch.zeros((cap, 160), dtype=torch.uint8, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
    return recs, cnt, gf_event_ring(recs.data_ptr(), cap, cnt.data_ptr())


def _ring_check(recs, cnt, e, what):
    n = int(cnt.item())
    assert n == len(e), f"{what}: {n} records vs {len(e)}"
    got = recs[:n].cpu().numpy()
    bad = np.nonzero((got != e).any(axis=1))[0]
    assert len(bad) == 0, f"{what}: {len(bad)} records differ, first {bad[:1]}: {got[bad[0]][:40]} vs {e[bad[0]][:40]}"
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["A", "B"])
def test_gpu_kats(variant):
    """The KATs through gf_pipeline_classify_tunnel: records, snap_out, tunnel_ip; and the event ring
    with GF_NETDEV_F_TRACE_NOTIFY (TRACE_FROM_STACK, TRACE_TO_OVERLAY after it for the encap redirects,
    the drops) against the model's list."""
    _gpu()
    import ctypes as C
    from cilium_amd._lib import lib
    from cilium_amd.datapath import Datapath
    sc, cases, want, wantf, wtun = kat_scenario(variant, flags=OPTS | synth.NETDEV_TRACE_NOTIFY)
    model = NM.NetdevModel(sc)
    ref = OracleDP(sc)
    wm, _, fm, _, front, (dl, sub) = model_run(sc, sc.batches[0], sc.now, ref, NM.pre_oracle(sc), model)
    assert (wm == want).all()
    fe = model.front_events(sc.batches[0], want, wantf)
    eps = {e["lxc_id"]: e for e in sc.lxc}
    ifx = {ep["lxc_id"]: ep["ifindex"] for ep in model.eps.values()}
    for i in np.nonzero((want["stage"] == 4) & (want["action"] == 2))[0]:   # handle_policy's drops (drop.h:47-107)
        e = eps[int(want["lxc_id"][i])]
        fe[i].append(NM.event(1 | (int(want["reason"][i]) << 8) | (e["lxc_id"] << 16), int(sc.batches[0].lens[i]),
                              int(model.secctx[i]) & 0xffff, e["seclabel"], e["lxc_id"], ifx[e["lxc_id"]], wantf[i]))
    exp = np.stack([r for ev in fe for r in ev])
    assert (exp[:, 0] == 4).sum() == len(cases) + int((wtun != 0).sum())
    recs, cnt, ring = _ring(1024)
    dp = Datapath(sc, pin_prefix=None)
    assert lib.gf_set_event_ring(C.byref(ring)) == 0
    try:
        got, nd6, snap, tun = _gpu_pipe(dp, sc.batches[0], sc.now)
        for k, c in enumerate(cases):
            assert got[k] == want[k], (c["name"], got[k], want[k])
            assert bytes(snap[k]) == bytes(wantf[k]), c["name"]
            assert tun[k] == wtun[k], (c["name"], hex(tun[k]))
        assert not nd6.any()
        _ring_check(recs, cnt, exp, "events")
    finally:
        lib.gf_set_event_ring(None)
        dp.close()


@pytest.mark.gpu
def test_gpu_options_off_is_todays_pipeline():
    """pipeline_fuzz through a pipeline loaded without the flags (gf_node_cfg.encap_ifindex set, a tunnel
    map present): gf_pipeline_classify, then gf_pipeline_classify_tunnel with tunnel_ip NULL on a second
    datapath; records, new_daddr6, frames, every CT / policy / proxy map and the event ring equal the
    oracle's; with a tunnel_ip column it comes back all 0."""
    _gpu()
    import ctypes as C
    from cilium_amd._lib import lib
    from cilium_amd.datapath import Datapath, DeviceBatch, to_numpy
    sc = synth.host_fuzz(seed=3, n_packets=6000, n_batches=2)     # pipeline_fuzz + remote pods, node encap config
    sc.host = None
    assert sc.node["encap_ifindex"] and sc.netdev["flags"] == 0
    for k, e in enumerate(sc.lxc):
        if k % 3 == 0:
            e["flags"] |= synth.LXC_TRACE_NOTIFY
    sc.netdev = dict(sc.netdev, flags=synth.NETDEV_TRACE_NOTIFY, ingress_ifindex=7)
    names = ["ct4", "ct6", "cilium_proxy4", "cilium_proxy6"] + [e["policy"] for e in sc.lxc]
    recs, cnt, ring = _ring()
    try:
        for call in ("classify", "tunnel_null", "tunnel_col"):
            if call == "tunnel_col":                    # without the prefilter the remote-pod frames reach from_netdev
                sc = copy.copy(sc)
                sc.xdp = None
            dp, ref = Datapath(sc, pin_prefix=None), OracleDP(sc)
            cnt.zero_()
            assert lib.gf_set_event_ring(C.byref(ring)) == 0
            exp = []
            for bi, pk in enumerate(sc.batches):
                if call == "classify":
                    out, nd6, snap = dp.pipeline(DeviceBatch(pk, parse=False), sc.now + bi)
                    torch.cuda.synchronize()
                    got, nd6, snap, tun = to_numpy(out, PIPE_OUT), nd6.cpu().numpy(), snap.cpu().numpy(), None
                else:
                    got, nd6, snap, tun = _gpu_pipe(dp, pk, sc.now + bi, tunnel_ip=call == "tunnel_col")
                with O.TraceSink(pk.n) as ts:
                    ro, rn6, rs = ref.pipeline(pk, sc.now + bi)
                _same(got, ro, f"{call} b{bi}")
                assert np.array_equal(nd6, rn6) and not (snap != rs).any(), f"{call} b{bi}"
                assert tun is None or not tun.any()
                in_cluster = (pk.frames[:, 12] == 0x08) & (pk.lens >= 34) & (pk.frames[:, 30] == 10) & (pk.frames[:, 31] == 77)
                assert in_cluster.sum() > 20 and not (got["flags"] & 0x0c).any() and not got["pad0"].any()
                if call == "tunnel_col":                # to the stack, as today, although encap_ifindex is set
                    m = in_cluster & (ro["stage"] == 3)     # (bpf_lb ends a few: checksum fields outside the frame)
                    assert m.sum() > 20 and (ro["action"][m] == 0).all()
                exp.append(ts.events())
            for name in names:
                assert dp.dump_map(name) == ref.dump(name), (call, name)
            _ring_check(recs, cnt, np.concatenate(exp), call)
            lib.gf_set_event_ring(None)
            dp.close()
    finally:
        lib.gf_set_event_ring(None)


@pytest.mark.gpu
def test_gpu_encap_equals_from_host():
    """The encap path against gf_host_classify, tested on its own: no XDP / LB program, marks 0, empty
    proxy maps, GF_NETDEV_F_ENCAP (HANDLE_NS off: the from-host program has no responders).  TCP / UDP
    frames too short for their ports are left out (reverse_proxy ends them in the from-host front).
    Records and tunnel_ip equal from-host's with stage 7 -> 3, daddr4 -> tunnel_ip and the encap flag;
    frames are equal except the destination MAC rewrite_dmac_to_host writes."""
    _gpu()
    from cilium_amd.datapath import Datapath, DeviceBatch, to_numpy
    sc = synth.host_fuzz(seed=4, n_packets=6000, n_batches=1, reverse=0.0)
    pk = sc.batches[0]
    f, ln = pk.frames, pk.lens.astype(np.int64)
    v4 = (f[:, 12] == 0x08) & (f[:, 13] == 0) & (ln >= 34)
    v6 = (f[:, 12] == 0x86) & (f[:, 13] == 0xDD) & (ln >= 54)
    l4 = np.where(v4, 14 + (f[:, 14] & 0xf).astype(np.int64) * 4, 54)
    nh = np.where(v4, f[:, 23], f[:, 20])
    pk = _subset(pk, ~((v4 | v6) & np.isin(nh, (6, 17)) & (l4 + 4 > ln)))
    sc.batches[0] = pk
    sc.xdp = sc.lb = None
    assert not sc.maps["cilium_proxy4"].n() and not sc.maps["cilium_proxy6"].n()
    sc.netdev = dict(sc.netdev, flags=sc.netdev["flags"] | synth.NETDEV_ENCAP, ingress_ifindex=5)
    sc.host = dict(sc.host, flags=sc.netdev["flags"] & 1)
    net_mac = np.frombuffer(sc.host["cilium_net_mac"], np.uint8)
    hs, nds = copy.copy(sc), copy.copy(sc)
    hs.netdev, nds.host = None, None
    dph = Datapath(hs, pin_prefix=None)
    b = DeviceBatch(pk, parse=False)
    b.mark = None
    ho, hsnap = dph.from_host(b, sc.now)
    torch.cuda.synchronize()
    ho, hsnap = to_numpy(ho, PIPE_OUT).copy(), hsnap.cpu().numpy()
    names = ["ct4", "ct6", "cilium_proxy4", "cilium_proxy6"] + [e["policy"] for e in sc.lxc]
    hd = {name: dph.dump_map(name) for name in names}
    dph.close()                                         # the node config is one per process
    dpn = Datapath(nds, pin_prefix=None)
    got, nd6, snap, tun = _gpu_pipe(dpn, pk, sc.now)
    enc = (ho["stage"] == 7) & (ho["action"] == 7) & (ho["flags"] & 0x20 == 0)
    assert enc.sum() > 100 and (ho["daddr4"][enc] != 0).all() and not ho["daddr4"][~enc].any()
    want = ho.copy()
    want["stage"][ho["stage"] == 7] = 3
    want["daddr4"] = 0
    want["flags"][enc] |= 0x08
    _same(got, want, "records")
    assert np.array_equal(tun, ho["daddr4"])
    # rewrite_dmac_to_host's six bytes: where from-host left CILIUM_NET_MAC, from_netdev left the frame's own
    dm = (hsnap[:, 0:6] == net_mac).all(axis=1) & (v4 | v6)[~((v4 | v6) & np.isin(nh, (6, 17)) & (l4 + 4 > ln))]
    exp = hsnap.copy()
    exp[dm, 0:6] = pk.frames[dm, 0:6]
    assert dm.sum() > enc.sum() and not (snap != exp).any()
    for name in names:
        assert dpn.dump_map(name) == hd[name], name
    dpn.close()


@pytest.mark.gpu
@pytest.mark.parametrize("stride,kind", [(128, "plain"), (256, "plain"), (122, "plain"), (256, "ctoff"), (122, "ctoff")])
def test_gpu_netdev_fuzz(stride, kind):
    """netdev_fuzz (the project's v4 / v6 mix, NS / echo frames, remote pods, truncated frames, extension
    headers) against the model: records, new_daddr6, frames, tunnel_ip, the CT / policy / proxy maps of
    the delivered subset and the event ring with GF_NETDEV_F_TRACE_NOTIFY, with global CT and with a
    CT-off endpoint in the array, on the uint4 path at both tile sizes and the byte path (122).
    The ring's expected content: the model's own records for the frames an option decided; for every
    other frame the list of an oracle pipeline that is given the same batch with those frames replaced
    by ARP (which from_netdev passes on without state), so that its CT state is the model's."""
    _gpu()
    import ctypes as C
    from cilium_amd._lib import lib
    from cilium_amd.datapath import Datapath
    events = kind == "plain"
    sc, off = fuzz_scenario(3, kind, stride=stride, trace=events)
    ref, pre, model = OracleDP(sc), NM.pre_oracle(sc), NM.NetdevModel(sc)
    ctoff = CM.CtOffModel(sc) if off else None
    pk = sc.batches[0]
    want, wn6, frames, wtun, front, (dl, sub) = model_run(sc, pk, sc.now, ref, pre, model, ctoff, off)
    recs, cnt, ring = _ring()
    dp = Datapath(sc, pin_prefix=None)
    if events:
        assert lib.gf_set_event_ring(C.byref(ring)) == 0
    try:
        got, nd6, snap, tun = _gpu_pipe(dp, pk, sc.now)
        _same(got, want, "records")
        assert np.array_equal(nd6, wn6) and np.array_equal(tun, wtun)
        cmp = _frames_cmp(pk, want)
        assert (want["stage"][~cmp] == 4).all()
        _frames_same(snap, frames, cmp, want, "frames")
        ct = sorted({e[k] for e in sc.lxc for k in ("ct4", "ct6") if e.get(k)})
        for name in ct + ["cilium_proxy4", "cilium_proxy6"]:
            assert dp.dump_map(name) == ref.dump(name), name
        for e in sc.lxc:
            w = ctoff.progs[e["lxc_id"]].policy_dump() if e["lxc_id"] in off else ref.dump(e["policy"])
            assert dp.dump_map(e["policy"]) == w, e["policy"]
        if events:
            sub_sc = copy.copy(sc)
            sub_sc.netdev = dict(sc.netdev, flags=sc.netdev["flags"] & 3)
            fr = pk.frames.copy()
            fr[model.opt, 12:14] = (0x08, 0x06)
            evo = OracleDP(sub_sc)
            with O.TraceSink(pk.n) as ts:
                ro, _, rs = evo.pipeline(Packets(fr, pk.lens, pk.src_identity, pk.ifindex, pk.lxc_id, pk.tc_index,
                                                 pk.flow_hash), sc.now)
            assert (ro[~model.opt] == want[~model.opt]).all() and not (rs[~model.opt] != snap[~model.opt]).any()
            fe = model.front_events(pk, want, frames)
            exp = [np.stack(fe[i]) if model.opt[i] else ts.ev[i, :ts.cnt[i]] for i in range(pk.n)]
            exp = np.concatenate([e for e in exp if len(e)])
            g = _ring_check(recs, cnt, exp, "events")
            assert ((g[:, 0] == 4) & (g[:, 1] == 4)).sum() == (wtun != 0).sum() > 20
    finally:
        lib.gf_set_event_ring(None)
        dp.close()


_EDGE = {}


def _edge_case():
    """257 netdev_fuzz frames whose every touched header byte lies in the first 128 bytes, and among
    them responder and encap frames to put first and last."""
    if not _EDGE:
        sc, _ = fuzz_scenario(6, "plain", n_packets=3000)
        pk = sc.batches[0]
        cols = OracleDP(sc).parse(pk)
        need = np.where(cols["proto"] == 6, 18, np.where(np.isin(cols["proto"], (17, 1, 58)), 8, 4))
        ip = np.isin(cols["ethertype"], (0x0800, 0x86DD))
        ok = ~ip | ((cols["l4_off"] >= 34) & (cols["l4_off"] + need <= 128))
        model = NM.NetdevModel(sc)
        rec = model.front(pk, NM.pre_oracle(sc), sc.now)[0]
        special = np.nonzero(ok & (rec["stage"] == 3) & (rec["flags"] & 0x0c != 0))[0]
        resp = special[rec["flags"][special] & 4 != 0]
        enc = special[rec["flags"][special] & 8 != 0]
        assert len(resp) > 2 and len(enc) > 2
        _EDGE.update(sc=sc, pk=_subset(pk, np.nonzero(ok)[0][:257]), resp=_subset(pk, resp[:2]), enc=_subset(pk, enc[:2]))
    return _EDGE


def _cat(*pks):
    c = lambda name: np.concatenate([getattr(p, name) for p in pks])
    return Packets(c("frames"), c("lens"), c("src_identity"), c("ifindex"), c("lxc_id"), c("tc_index"), c("flow_hash"))


@pytest.mark.gpu
@pytest.mark.parametrize("stride", [128, 144])
def test_gpu_tile_edges(stride):
    """n around the 128- and 256-lane tiles (stride 128: 256 lanes, uint4 path; 144: 128 lanes) with a
    responder frame first and an encap frame last, then the other way round, with and without snap_out
    and the tunnel_ip column, tc_index / flow_hash present or NULL, against the model; the calls run one
    after the other on one datapath and one oracle."""
    _gpu()
    from cilium_amd.datapath import Datapath
    E = _edge_case()
    sc = E["sc"]
    dp, ref, pre, model = Datapath(sc, pin_prefix=None), OracleDP(sc), NM.pre_oracle(sc), NM.NetdevModel(sc)
    k = 0
    for n in (1, 127, 128, 129, 255, 256, 257):
        for first, last in ((E["resp"], E["enc"]), (E["enc"], E["resp"])):
            mid = E["pk"].slice(0, max(n - 2, 0))
            pk = _cat(first.slice(0, 1), mid, last.slice(1, 2)) if n > 1 else first.slice(0, 1)
            assert pk.n == n
            snap_out, tunnel_ip, bare = ((True, True, False), (False, True, True), (True, False, True))[k % 3]
            k += 1
            pk = Packets(np.ascontiguousarray(pk.frames[:, :stride]), pk.lens, None, None, None,
                         None if bare else pk.tc_index, None if bare else pk.flow_hash)
            got, nd6, snap, tun = _gpu_pipe(dp, pk, sc.now, snap_out=snap_out, tunnel_ip=tunnel_ip, bare=bare)
            want, wn6, frames, wtun, _, _ = model_run(sc, pk, sc.now, ref, pre, model)
            _same(got, want, f"n {n} stride {stride}")
            assert want["flags"][0] & 0x0c and want["flags"][-1] & 0x0c
            assert np.array_equal(nd6, wn6) and (tun is None or np.array_equal(tun, wtun))
            if snap_out:
                cmp = _frames_cmp(pk, want)
                assert not (snap[cmp] != frames[cmp]).any(), (n, stride)
    dp.close()


@pytest.mark.gpu
def test_gpu_respond_after_pipeline():
    """Datapath.respond_after over a pipeline batch: gf_respond_calls takes the call from the record
    (pad0) without the frames, the replies equal tests/respond_model.py's, an NS for an unknown target
    is TC_ACT_OK under GF_RESPOND_F_NS_TO_STACK (bpf_netdev.c:25), and the pipeline's own records and
    frames equal a run without the responder call."""
    _gpu()
    import ctypes as C
    from cilium_amd._lib import lib, gf_frames, GF_REC_PIPELINE, GF_RESPOND_F_NS_TO_STACK
    from cilium_amd.datapath import Datapath, DeviceBatch, to_numpy
    from tests import respond_model as RM
    sc, _ = fuzz_scenario(5, "plain", n_packets=3000, stride=128)
    pk = sc.batches[0]
    dp = Datapath(sc, pin_prefix=None)
    b = DeviceBatch(pk, parse=False)
    out, nd6, snap, tun = dp.pipeline_tunnel(b, sc.now)
    torch.cuda.synchronize()
    rec0, snap0 = to_numpy(out, PIPE_OUT).copy(), snap.cpu().numpy().copy()
    call, rout, reply = dp.respond_after(GF_REC_PIPELINE, b, out, snap, flags=GF_RESPOND_F_NS_TO_STACK)
    torch.cuda.synchronize()
    assert (to_numpy(out, PIPE_OUT) == rec0).all() and not (snap.cpu().numpy() != snap0).any()
    call = call.cpu().numpy()
    resp = rec0["flags"] & 0x04 != 0
    te = (rec0["flags"] & 0x20 != 0) & (rec0["stage"] != 4)
    assert (call[resp] == rec0["pad0"][resp]).all() and (call[te] == 4).all() and not call[~(resp | te)].any()
    assert (call == 2).any() and (call == 3).any()
    # the call column needs no frames: a NULL snap gives the same column
    c2 = torch.empty(pk.n, dtype=torch.uint8, device="cuda")
    fr = gf_frames(pk.n, 128, None, b.len.data_ptr())
    assert lib.gf_respond_calls(C.byref(fr), out.data_ptr(), GF_REC_PIPELINE, c2.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert np.array_equal(c2.cpu().numpy(), call)
    rout = to_numpy(rout, RM.RESP_OUT)
    reply = reply.cpu().numpy()
    nd = sc.node
    cfg = RM.Cfg(struct.pack("<I", nd.get("ipv4_gateway", 0)), nd["router_ip6"], nd["node_mac"], flags=RM.F_NS_TO_STACK)
    frames = np.where((call == 4)[:, None], snap0, pk.frames)
    mrec, msnap, _ = RM.respond(cfg, frames, pk.lens, call, None, None, None)
    assert np.array_equal(rout, mrec)
    live = call != 0
    assert np.array_equal(reply[live], msnap[live])
    unknown = resp & (call == 2) & (pk.lens >= 78) & (pk.frames[:, 62:78] != np.frombuffer(nd["router_ip6"], np.uint8)).any(axis=1)
    assert unknown.any() and (rout["action"][unknown] == 0).all() and not (reply[unknown] != pk.frames[unknown]).any()
    assert (rout["action"][resp & (call == 2)] == 7).any() and (rout["action"][resp & (call == 3)] == 7).any()
    dp.close()
