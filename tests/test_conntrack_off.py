"""The Conntrack endpoint option disabled — GF_LXC_F_NO_CONNTRACK
(pkg/endpoint/endpoint.go:111-114: CONNTRACK undefined; bpf/lib/conntrack.h:582-617:
ct_lookup / ct_create / ct_delete are empty stubs).  The reference's
RuntimeValidatedConntrackTest ends on this leg (test/runtime/connectivity.go:690-709).

The CPU oracle cannot express the option, so the check is tests/ctoff_model.py (a
per-packet restatement of handle_policy with the stubs) for the packets of CT-off
programs and the unchanged oracle for everything else: the CT-on packets of a mixed
array as a sub-batch in their original order, and every CT-off packet that never
reaches ipv4_policy / ipv6_policy.

The pipeline's CT-off packets get the model's handle_policy over what bpf_netdev hands
to it: the frame as the earlier programs left it (from an oracle run in which the CT-off
endpoints are DROP_ALL, so that their handle_policy writes nothing), the source identity
and ifindex restated in ctoff_model.netdev_inputs.  gf_lxc_egress_classify refuses arrays
with a CT-off program (-EOPNOTSUPP).
"""
import errno
import ipaddress
import json
import os
import struct

import numpy as np
import pytest

from cilium_amd import synth
from cilium_amd.synth import Packets
from oracle.scenario import OracleDP
from tests import ctoff_model as M
from tests import runtime_matrix as RM

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KAT_IFINDEX, KAT_HOST_IFINDEX, KAT_NOW = 11, 3, 5000


def _subset(pk, m):
    f = lambda x: None if x is None else x[m]
    return Packets(pk.frames[m], pk.lens[m], f(pk.src_identity), f(pk.ifindex), f(pk.lxc_id), f(pk.tc_index),
                   f(pk.flow_hash))


def _raw16(x):
    return ((x & 0xff) << 8) | (x >> 8)


# ---------------------------------------------------------------- KATs
def _kats():
    with open(os.path.join(GOLDEN, "ctoff_kats.json")) as f:
        return json.load(f)["cases"]


def kat_scenario():
    """One endpoint and one packet per KAT.  Every program is given the CT maps next to
    the flag (they are to be ignored); 'ct_prefill' cases have their reply entry there.
    Returns (scenario, expected ING_OUT records, expected cilium_proxy4/6 contents)."""
    cases = _kats()
    sc = synth.Scenario("ctoff_kats", now=KAT_NOW, host_ifindex=KAT_HOST_IFINDEX)
    gw = 0xfffff50a
    host6 = bytes([0xbe, 0xef, 0, 0, 0, 0, 0, 0, 0, 0, 0xa, 0, 0x2, 0xf, 0xff, 0xff])
    sc.add_map(synth.MapSpec("cilium_proxy4", synth.HASH, 10, 16, 4096, 0))
    sc.add_map(synth.MapSpec("cilium_proxy6", synth.HASH, 22, 28, 4096, 0))
    sc.node = {"proxy4": "cilium_proxy4", "proxy6": "cilium_proxy6", "ipv4_gateway": gw, "host_ip6": host6,
               "host_mac": bytes([0xce, 0x72, 0xa7, 0x03, 0x88, 0x56]), "node_mac": bytes([0xde, 0xad, 0xbe, 0xef, 0xc0, 0xde])}
    ct4k, ct4v, ct6k, ct6v = [], [], [], []
    frames, lens, sid, lid, tci = [], [], [], [], []
    want = np.zeros(len(cases), M.ING_OUT)
    px4, px6 = {}, {}
    protos = {"tcp": synth.TCP, "udp": synth.UDP}
    for k, c in enumerate(cases):
        v6 = c["family"] == 6
        ep4 = synth.ip4("10.1.0.1") + k
        ep6 = ipaddress.IPv6Address(int(ipaddress.IPv6Address("f00d::a0f:0:0:0")) + 1 + k).packed
        p = c["packet"]
        nh = protos[p["proto"]]
        flags = synth.LXC_POLICY_INGRESS | synth.LXC_LXC_IPV4 | synth.LXC_NO_CONNTRACK
        if "HAVE_L4_POLICY" in c["flags"]:
            flags |= synth.LXC_HAVE_L4_POLICY
        pol = np.array(c["policy"], np.uint32).reshape(-1, 4)
        pk_, pv_ = (synth.policy_keys(pol[:, 0], pol[:, 1], pol[:, 2]), synth.policy_vals(pol[:, 3])) if len(pol) else (None, None)
        sc.add_map(synth.MapSpec(f"pol{k}", synth.HASH, 8, 24, 1024, 0, pk_, pv_))
        e = {"lxc_id": 3000 + k, "seclabel": 500 + k, "policy": f"pol{k}", "ct4": "ct4", "ct6": "ct6", "flags": flags,
             "l4": []}
        for cidr in c.get("cidr", []):
            net = ipaddress.ip_network(cidr)
            if net.version == 4:
                ck = synth.lpm4_keys(np.array([net.prefixlen], np.uint32), np.array([int(net.network_address)], np.uint32))
                sc.add_map(synth.MapSpec(f"cidr4_{k}", synth.LPM, 8, 1, 64, synth.NO_PREALLOC, ck, np.ones((1, 1), np.uint8)))
                e["cidr4"] = f"cidr4_{k}"
            else:
                ck = synth.lpm6_keys(np.array([net.prefixlen], np.uint32),
                                     np.frombuffer(net.network_address.packed, np.uint8)[None])
                sc.add_map(synth.MapSpec(f"cidr6_{k}", synth.LPM, 20, 1, 64, synth.NO_PREALLOC, ck, np.ones((1, 1), np.uint8)))
                e["cidr6"] = f"cidr6_{k}"
        sc.lxc.append(e)
        tf = p.get("tcp_flags", synth.F_SYN)
        if v6:
            src = np.frombuffer(ipaddress.IPv6Address(p["src"]).packed, np.uint8)
            f, ln = synth.frames_v6(1, 128, src[None], np.frombuffer(ep6, np.uint8)[None], nh, p["sport"], p["dport"], tf)
            l4 = 54
        else:
            f, ln = synth.frames_v4(1, 128, synth.ip4(p["src"]), ep4, nh, p["sport"], p["dport"], tf)
            l4 = 34
        if "l4_keep" in p:
            ln = np.array([l4 + p["l4_keep"]], np.uint32)
        if c.get("ct_prefill"):
            if v6:
                ct6k.append(synth.pack_rows(np.frombuffer(ep6, np.uint8)[None], src[None],
                                            synth.le_bytes(synth.raw16([p["sport"]]), "<u2"),
                                            synth.le_bytes(synth.raw16([p["dport"]]), "<u2"),
                                            np.full((1, 1), nh, np.uint8), np.zeros((1, 3), np.uint8)))
                ct6v.append(synth.ct_vals(1, KAT_NOW + 4000, 16, 0, 300))
            else:
                ct4k.append(synth.ct4_keys([ep4], [synth.ip4(p["src"])], synth.raw16([p["sport"]]), synth.raw16([p["dport"]]),
                                           [nh], [0]))
                ct4v.append(synth.ct_vals(1, KAT_NOW + 4000, 16, 0, 300))
        frames.append(f); lens.append(ln); sid.append(p["identity"]); lid.append(3000 + k); tci.append(p.get("tc_index", 0))
        x = c["expect"]
        want[k] = (x["action"], x["reason"], 0, x["flags"], _raw16(x["proxy_port"]), x["ifindex"])
        if "proxy_key" in c:
            q = c["proxy_key"]
            assert q["saddr"] == "endpoint" and q["orig_daddr"] == "endpoint"
            addr = ep6 if v6 else struct.pack(">I", ep4)
            key = addr + struct.pack("<HHBB", _raw16(q["dport"]), _raw16(q["sport"]), q["nexthdr"], 0)
            val = addr + struct.pack("<HHII", _raw16(q["orig_dport"]), 0, q["identity"], KAT_NOW + 720)
            (px6 if v6 else px4)[key] = val
    cat = lambda a: np.concatenate(a) if a else None
    sc.add_map(synth.MapSpec("ct4", synth.LRU_HASH, 14, 48, 4096, 0, cat(ct4k), cat(ct4v)))
    sc.add_map(synth.MapSpec("ct6", synth.LRU_HASH, 40, 48, 4096, 0, cat(ct6k), cat(ct6v)))
    n = len(cases)
    sc.batches.append(Packets(np.concatenate(frames), np.concatenate(lens).astype(np.uint32), np.array(sid, np.uint32),
                              np.full(n, KAT_IFINDEX, np.uint32), np.array(lid, np.uint16), np.array(tci, np.uint8),
                              np.zeros(n, np.uint32)))
    return sc, want, px4, px6


def test_kats_cover_the_issue_table():
    names = [c["name"] for c in _kats()]
    assert len(names) == len(set(names)) == 18
    assert all(c.get("derivation") for c in _kats())
    assert sorted(n[:-3] for n in names if n.endswith("_v6")) == sorted(n for n in names if not n.endswith("_v6"))


def test_model_reproduces_every_kat():
    sc, want, px4, px6 = kat_scenario()
    pk = sc.batches[0]
    model = M.CtOffModel(sc)
    idx, got, reached = model.batch(pk, OracleDP(sc).parse(pk), sc.now)
    assert list(idx) == list(range(pk.n)) and reached.all()
    for k, c in enumerate(_kats()):
        assert got[k] == want[k], (c["name"], got[k], want[k])
    assert model.proxy4 == px4 and model.proxy6 == px6


def test_synth_conntrack_off_configs_pack():
    """synth.conntrack_off: flag set, CT bindings and L3L4 lists gone on every 2nd
    endpoint; the configs go through the gf_lxc_cfg packing of the datapath."""
    from cilium_amd._lib import gf_lxc_cfg
    from cilium_amd.datapath import egress_fields
    sc = synth.fuzz(seed=1, n_packets=100, n_batches=1)
    off = synth.conntrack_off(sc, every=2)
    assert off == [e["lxc_id"] for j, e in enumerate(sc.lxc) if j % 2 == 0]
    for j, e in enumerate(sc.lxc):
        is_off = j % 2 == 0
        assert bool(e["flags"] & synth.LXC_NO_CONNTRACK) == is_off
        if is_off:
            assert e["ct4"] is None and e["ct6"] is None and e["l4"] == []
        else:
            assert e["ct4"] == "ct4" and e["ct6"] == "ct6"
        cfg = gf_lxc_cfg()
        cfg.flags, cfg.lxc_id = e["flags"], e["lxc_id"]
        cfg.ct_map4 = 0 if e["ct4"] is None else 7
        cfg.n_l4_ingress = len(e["l4"])
        egress_fields(cfg, e, lambda name: 0)
        assert cfg.flags & 128 == (128 if is_off else 0) and (cfg.ct_map4 == 0) == is_off
    # the model accepts exactly the CT-off endpoints
    assert sorted(M.CtOffModel(sc).progs) == sorted(off)


def test_prog_load_refuses_l3l4_lists_without_conntrack():
    """CFG_L3L4_* requires CONNTRACK (bpf/lib/l4.h:138-139): -EINVAL, checked before
    any map is looked at (the library loads without a device)."""
    import ctypes as C
    from cilium_amd._lib import lib, gf_lxc_cfg
    for field in ("n_l4_ingress", "n_l4_egress"):
        cfg = gf_lxc_cfg()
        cfg.flags = synth.LXC_PRODUCTION | synth.LXC_NO_CONNTRACK
        setattr(cfg, field, 1)
        assert lib.gf_lxc_prog_load(C.byref(cfg)) == -errno.EINVAL, field


def _runtime_doc():
    with open(os.path.join(GOLDEN, "runtime_conntrack_off.json")) as f:
        return json.load(f)


def runtime_leg(without_reverse):
    """connectivity.go:690-709 ingress-only: every packet of every request as one
    handle_policy batch at its receiver (cb[CB_SRC_LABEL] = the sender's identity).
    Returns (scenario, packets, [to_client?])."""
    doc = _runtime_doc()
    case = json.loads(json.dumps(doc["case"]))
    if without_reverse:
        drop = doc["without_reverse_rule"]["drop_from_client_ingress"]
        rule = [r for r in case["rules"] if r["select"] == "id.client"][0]
        rule["ingress"][0]["fromEndpoints"].remove(drop)
    topo = RM.Topology(doc["endpoints"])
    sc = RM.compile_case(case, topo)
    off = synth.conntrack_off(sc)
    assert sorted(off) == sorted(topo.lxc_id[n] for n in doc["conntrack_off"])
    rows = []
    for j, (c, s, r, ok) in enumerate(RM.expand(case)):
        assert ok
        f = RM.Flow(j, c, s, r)
        for step in range(len(f.steps)):
            fr, ln, src, dst = RM._frame(topo, f, step)
            rows.append((fr, ln, src, dst))
    pk = Packets(np.concatenate([x[0] for x in rows]), np.concatenate([x[1] for x in rows]).astype(np.uint32),
                 np.array([topo.ident[x[2]] for x in rows], np.uint32), np.array([topo.ifindex[x[3]] for x in rows], np.uint32),
                 np.array([topo.lxc_id[x[3]] for x in rows], np.uint16), np.zeros(len(rows), np.uint8),
                 np.zeros(len(rows), np.uint32))
    return sc, pk, np.array([x[3] == "client" for x in rows])


def check_runtime_leg(records, to_client, without_reverse):
    assert to_client.any() and (~to_client).any()
    assert (records["action"][~to_client] != 2).all(), "a request did not reach the server"
    if without_reverse:
        assert (records["action"][to_client] == 2).all() and (records["reason"][to_client] == 133).all()
    else:
        assert (records["action"][to_client] != 2).all(), "a reply did not reach the client"
    assert (records["ct_ret"] == 0).all()


@pytest.mark.parametrize("without_reverse", [False, True])
def test_model_runtime_leg(without_reverse):
    sc, pk, to_client = runtime_leg(without_reverse)
    idx, rec, reached = M.CtOffModel(sc).batch(pk, OracleDP(sc).parse(pk), sc.now)
    assert len(idx) == pk.n and reached.all()
    check_runtime_leg(rec, to_client, without_reverse)


def mixed_scenario(seed, every, mx, local=True):
    sc = synth.fuzz(seed=seed, n_packets=20000, n_batches=3, ct_max=mx or 100000, ct6_max=mx or 100000)
    off = synth.conntrack_off(sc, every=every)
    made = []
    if local:                                           # ConntrackLocal on every 2nd of the endpoints that keep conntrack
        full = sc.lxc
        sc.lxc = [e for e in full if e["lxc_id"] not in off]
        made = synth.conntrack_local(sc, every=2, max_entries=mx)
        sc.lxc = full
    return sc, off, made


def split_check(sc, off, got_recs, ref, model, mixed):
    """got_recs[bi]: the ING_OUT records of batch bi.  CT-off packets against the
    model, the rest against the oracle run on them alone; returns the model's counts
    (cover = [ct-off packets, others, reached+allowed, reached+dropped])."""
    cover = np.zeros(4, np.int64)
    for bi, pk in enumerate(sc.batches):
        now = sc.now + bi
        got = got_recs[bi]
        idx, mrec, reached = model.batch(pk, ref.parse(pk), now)
        offm = np.zeros(pk.n, bool)
        offm[idx] = True
        assert np.array_equal(offm, np.isin(pk.lxc_id, off))
        bad = np.nonzero(got[idx] != mrec)[0]
        assert len(bad) == 0, f"batch {bi}: {len(bad)} CT-off records differ from the model, first packet {idx[bad[:1]]}: " \
                              f"{got[idx][bad[:1]]} != {mrec[bad[:1]]}"
        want_on = ref.ingress(_subset(pk, ~offm), now)
        bad = np.nonzero(got[~offm] != want_on)[0]
        assert len(bad) == 0, f"batch {bi}: {len(bad)} CT-on records differ from the oracle"
        # CT-off packets that never reach ipv{4,6}_policy do not depend on CT: the oracle agrees
        nr = idx[~reached]
        assert np.array_equal(ref.ingress(_subset(pk, nr), now, lru=False), mrec[~reached])
        cover += (len(idx), pk.n - len(idx), int((reached & (mrec["action"] != 2)).sum()),
                  int((reached & (mrec["reason"] == M.DROP_POLICY)).sum()))
    if mixed:
        total = cover[0] + cover[1]
        assert cover[0] * 4 >= total and cover[1] * 4 >= total, cover
        assert cover[2] >= 100 and cover[3] >= 100, cover
    return cover


@pytest.mark.parametrize("seed,every", [(1, 2), (2, 3), (3, 2), (4, 2)])
def test_mixed_split_is_not_thin(seed, every):
    """The coverage condition of the GPU cases, on the CPU: each side at least a quarter
    of the batch, at least 100 CT-off packets allowed and 100 dropped by policy."""
    sc, off, _ = mixed_scenario(seed, every, None, local=False)
    model, ref = M.CtOffModel(sc), OracleDP(sc)
    cover = np.zeros(4, np.int64)
    for bi, pk in enumerate(sc.batches):
        idx, mrec, reached = model.batch(pk, ref.parse(pk), sc.now + bi)
        cover += (len(idx), pk.n - len(idx), int((reached & (mrec["action"] != 2)).sum()),
                  int((reached & (mrec["reason"] == M.DROP_POLICY)).sum()))
    total = cover[0] + cover[1]
    assert cover[0] * 4 >= total and cover[1] * 4 >= total and cover[2] >= 100 and cover[3] >= 100, cover


# ---------------------------------------------------------------- GPU
torch = pytest.importorskip("torch")


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(0)


def _gpu_ingress(dp, sc, batches_api=False):
    from cilium_amd.datapath import DeviceBatch, ING_OUT, to_numpy
    if batches_api:
        outs = dp.ingress_batches([DeviceBatch(pk) for pk in sc.batches], [sc.now + k for k in range(len(sc.batches))])
        torch.cuda.synchronize()
        return [to_numpy(o, ING_OUT) for o in outs]
    recs = []
    for bi, pk in enumerate(sc.batches):
        io = dp.ingress(DeviceBatch(pk), sc.now + bi)
        torch.cuda.synchronize()
        recs.append(to_numpy(io, ING_OUT))
    return recs


def _policy_maps_check(sc, off, dp, ref, model):
    for e in sc.lxc:
        name = e["policy"]
        want = model.progs[e["lxc_id"]].policy_dump() if e["lxc_id"] in off else ref.dump(name)
        assert dp.dump_map(name) == want, name


@pytest.mark.gpu
@pytest.mark.parametrize("batches_api", [False, True])
def test_gpu_all_endpoints_ct_off(batches_api):
    """Every program CT-off (k_ing_noct alone, no schedule): records equal the model,
    policy maps equal start + the model's counter deltas, and the CT maps — given to
    the programs next to the flag and prefilled with entries that match as REPLY /
    ESTABLISHED — stay byte-identical: they are not consulted."""
    _gpu()
    from cilium_amd.datapath import Datapath
    sc = synth.fuzz(seed=1, n_packets=20000, n_batches=3)
    off = synth.conntrack_off(sc)
    for e in sc.lxc:
        e["ct4"], e["ct6"] = "ct4", "ct6"               # may be given: ignored with the flag
    pre4 = {bytes(k): bytes(v) for k, v in zip(sc.maps["ct4"].keys, sc.maps["ct4"].vals)}
    pre6 = {bytes(k): bytes(v) for k, v in zip(sc.maps["ct6"].keys, sc.maps["ct6"].vals)}
    dp, ref, model = Datapath(sc, pin_prefix=None), OracleDP(sc), M.CtOffModel(sc)
    cover = split_check(sc, off, _gpu_ingress(dp, sc, batches_api), ref, model, False)
    assert cover[2] >= 100 and cover[3] >= 100, cover
    _policy_maps_check(sc, off, dp, ref, model)
    assert dp.dump_map("ct4") == pre4 and dp.dump_map("ct6") == pre6
    dp.close()


@pytest.mark.gpu
@pytest.mark.parametrize("seed,every,mx,batches_api", [(1, 2, None, False), (2, 3, None, False), (3, 2, 700, False),
                                                       (4, 2, None, True)])
def test_gpu_mixed_ct_off(seed, every, mx, batches_api):
    """CT-off programs beside global-map and ConntrackLocal programs (mx: small maps,
    the LRU eviction runs beside CT-off traffic): CT-off records equal the model, the
    others and every CT map equal the oracle run on the CT-on packets alone."""
    _gpu()
    from cilium_amd.datapath import Datapath
    sc, off, made = mixed_scenario(seed, every, mx)
    dp, ref, model = Datapath(sc, pin_prefix=None), OracleDP(sc), M.CtOffModel(sc)
    split_check(sc, off, _gpu_ingress(dp, sc, batches_api), ref, model, True)
    _policy_maps_check(sc, off, dp, ref, model)
    for name in made + ["ct4", "ct6"]:
        assert dp.dump_map(name) == ref.dump(name), name
    dp.close()


@pytest.mark.gpu
def test_gpu_kats():
    _gpu()
    from cilium_amd.datapath import Datapath
    sc, want, px4, px6 = kat_scenario()
    pre4 = {bytes(k): bytes(v) for k, v in zip(sc.maps["ct4"].keys, sc.maps["ct4"].vals)}
    pre6 = {bytes(k): bytes(v) for k, v in zip(sc.maps["ct6"].keys, sc.maps["ct6"].vals)}
    assert pre4 and pre6
    dp = Datapath(sc, pin_prefix=None)
    got = _gpu_ingress(dp, sc)[0]
    for k, c in enumerate(_kats()):
        assert got[k] == want[k], (c["name"], got[k], want[k])
    assert dp.dump_map("cilium_proxy4") == px4 and dp.dump_map("cilium_proxy6") == px6
    assert dp.dump_map("ct4") == pre4 and dp.dump_map("ct6") == pre6     # neither consulted nor written
    dp.close()


@pytest.mark.gpu
def test_gpu_proxy_redirects_all_off():
    """CT-off endpoints with proxy_port entries at dport 0: cilium_proxy4 / 6 equal
    the model's inserts (two packets with one key in a batch write equal values)."""
    _gpu()
    from cilium_amd.datapath import Datapath
    sc = synth.fuzz(seed=6, n_packets=4000, n_batches=2)
    sc.add_map(synth.MapSpec("cilium_proxy4", synth.HASH, 10, 16, 65536, 0))
    sc.add_map(synth.MapSpec("cilium_proxy6", synth.HASH, 22, 28, 65536, 0))
    sc.node = {"proxy4": "cilium_proxy4", "proxy6": "cilium_proxy6", "ipv4_gateway": 0xfffff50a,
               "host_ip6": bytes(range(16))}
    off = synth.conntrack_off(sc)
    for j, e in enumerate(sc.lxc):                      # {id, 0, proto} entries with a proxy port
        m = sc.maps[e["policy"]]
        ids = np.array([1, 2, 256, 257, 258, 259], np.uint32)
        k = synth.policy_keys(ids, np.zeros(6), np.array([6, 17, 6, 17, 1, 58]))
        v = synth.policy_vals(np.array([9000 + j, 0, 9100 + j, 9200, 9300, 9400]))
        m.keys, m.vals = synth.dedup(np.concatenate([k, m.keys]), np.concatenate([v, m.vals]))
    dp, ref, model = Datapath(sc, pin_prefix=None), OracleDP(sc), M.CtOffModel(sc)
    split_check(sc, off, _gpu_ingress(dp, sc), ref, model, False)
    assert len(model.proxy4) > 20 and len(model.proxy6) > 5
    # lifetime = the last writer's now + 720: per key the model keeps the last write in batch order
    assert dp.dump_map("cilium_proxy4") == model.proxy4
    assert dp.dump_map("cilium_proxy6") == model.proxy6
    _policy_maps_check(sc, off, dp, ref, model)
    dp.close()


def pipeline_scenario(seed, every, local):
    """pipeline_fuzz with CT-off endpoints that hold no proxy_port entries (cilium_proxy4 / 6
    are shared with the CT-on half, whose oracle run then stays valid for them), and the
    same scenario with those endpoints DROP_ALL instead: its oracle run gives every frame
    as it reaches handle_policy (DROP_ALL returns before any write, bpf_lxc.c:986-989)."""
    import copy
    sc = synth.pipeline_fuzz(seed=seed, n_packets=20000, n_batches=3)
    off = synth.conntrack_off(sc, every=every)
    for e in sc.lxc:
        if e["lxc_id"] in off:
            sc.maps[e["policy"]].vals[:, 0:2] = 0
    made = []
    if local:
        full = sc.lxc
        sc.lxc = [e for e in full if e["lxc_id"] not in off]
        made = synth.conntrack_local(sc, every=2)
        sc.lxc = full
    front = copy.copy(sc)
    front.lxc = [dict(e, flags=(e["flags"] & ~synth.LXC_NO_CONNTRACK) | synth.LXC_DROP_ALL) if e["lxc_id"] in off else e
                 for e in sc.lxc]
    return sc, off, made, front


@pytest.mark.gpu
@pytest.mark.parametrize("seed,every,local", [(3, 1, False), (8, 2, True), (11, 3, True)])
def test_gpu_pipeline_ct_off(seed, every, local):
    """The full pipeline, every endpoint CT-off and mixed (with ConntrackLocal on the
    rest): the CT-off endpoints' stage-POLICY records and rewritten frames equal the
    model's, everything else — records, nd6, frames, every CT map, cilium_proxy4 / 6 —
    equals the oracle run on the other packets alone, in their original order."""
    _gpu()
    from cilium_amd.datapath import Datapath, DeviceBatch, PIPE_OUT, to_numpy
    sc, off, made, front_sc = pipeline_scenario(seed, every, local)
    dp, ref, front, model = Datapath(sc, pin_prefix=None), OracleDP(sc), OracleDP(front_sc), M.CtOffModel(sc)
    cover = np.zeros(4, np.int64)
    for bi, pk in enumerate(sc.batches):
        now = sc.now + bi
        out, nd6, snap = dp.pipeline(DeviceBatch(pk, parse=False), now)
        torch.cuda.synchronize()
        got, got6, gots = to_numpy(out, PIPE_OUT), nd6.cpu().numpy(), snap.cpu().numpy()
        fo, f6, fs = front.pipeline(pk, now, lru=False)
        offm = (fo["stage"] == 4) & np.isin(fo["lxc_id"], off)
        # CT-off: handle_policy of the model over bpf_netdev's hand-over
        sid, ifx, lid = M.netdev_inputs(sc, fs, offm)
        assert np.array_equal(lid[offm], fo["lxc_id"][offm])
        sub = Packets(fs[offm].copy(), pk.lens[offm], sid[offm], ifx[offm], lid[offm],
                      None if pk.tc_index is None else pk.tc_index[offm], None)
        idx, mrec, reached = model.batch(sub, ref.parse(sub), now, write_frames=True)
        assert len(idx) == sub.n
        want = fo[offm].copy()                          # the earlier programs' fields, then handle_policy's
        want["action"], want["reason"], want["ct_ret"] = mrec["action"], mrec["reason"], mrec["ct_ret"]
        want["flags"] = (want["flags"] & 0xE0) | mrec["flags"]
        want["proxy_port"], want["ifindex_lo"] = mrec["proxy_port"], mrec["ifindex_lo"]
        bad = np.nonzero(got[offm] != want)[0]
        assert len(bad) == 0, f"b{bi}: {len(bad)} CT-off records differ, first {got[offm][bad[:1]]} != {want[bad[:1]]}"
        assert np.array_equal(got6[offm], f6[offm]), f"nd6 (CT-off) b{bi}"
        assert not (gots[offm] != sub.frames).any(), f"frames (CT-off) b{bi}"
        # the rest: the oracle on the sub-batch
        on = _subset(pk, ~offm)
        ro, rn6, rs = ref.pipeline(on, now)
        assert np.array_equal(got[~offm], ro), f"pipeline (CT-on) b{bi}"
        assert np.array_equal(got6[~offm], rn6), f"nd6 (CT-on) b{bi}"
        assert not (gots[~offm] != rs).any(), f"frames (CT-on) b{bi}"
        cover += (int(offm.sum()), int((~offm & (fo["stage"] == 4)).sum()), int((reached & (mrec["action"] != 2)).sum()),
                  int((reached & (mrec["reason"] == M.DROP_POLICY)).sum()))
    assert cover[2] >= 100 and cover[3] >= 100, cover
    if every > 1:                                       # both sides of the split at the policy stage are well filled
        assert cover[0] * 4 >= cover[0] + cover[1] and cover[1] * 4 >= cover[0] + cover[1], cover
    _policy_maps_check(sc, off, dp, ref, model)
    for name in made + ["ct4", "ct6", "cilium_proxy4", "cilium_proxy6"]:
        assert dp.dump_map(name) == ref.dump(name), name
    assert not model.proxy4 and not model.proxy6
    dp.close()


@pytest.mark.gpu
def test_gpu_egress_refuses_ct_off_arrays():
    """One CT-off program in the array: gf_lxc_egress_classify returns -EOPNOTSUPP and
    changes no state."""
    _gpu()
    from cilium_amd.datapath import Datapath, DeviceBatch
    sc = synth.pipeline_fuzz(seed=3, n_packets=2000, n_batches=1)
    off = synth.conntrack_off(sc, every=len(sc.lxc))
    assert len(off) == 1
    dp = Datapath(sc, pin_prefix=None)
    names = ["ct4", "ct6", "cilium_proxy4", "cilium_proxy6"] + [e["policy"] for e in sc.lxc]
    before = {n: dp.dump_map(n) for n in names}
    b = DeviceBatch(sc.batches[0], parse=False)
    with pytest.raises(OSError) as ei:
        dp.egress(b, sc.now)
    assert ei.value.errno == errno.EOPNOTSUPP
    torch.cuda.synchronize()
    assert {n: dp.dump_map(n) for n in names} == before
    dp.close()


@pytest.mark.gpu
@pytest.mark.parametrize("without_reverse", [False, True])
def test_gpu_runtime_leg(without_reverse):
    """connectivity.go:690-709: Conntrack off on client and server, the both-directions
    L3 policy: requests and replies pass; without the client's rule for the server the
    replies are dropped (no packet is a reply without conntrack)."""
    _gpu()
    from cilium_amd.datapath import Datapath, DeviceBatch, ING_OUT, to_numpy
    sc, pk, to_client = runtime_leg(without_reverse)
    dp = Datapath(sc, pin_prefix=None)
    io = dp.ingress(DeviceBatch(pk), sc.now)
    torch.cuda.synchronize()
    got = to_numpy(io, ING_OUT)
    check_runtime_leg(got, to_client, without_reverse)
    _, want, _ = M.CtOffModel(sc).batch(pk, OracleDP(sc).parse(pk), sc.now)
    assert np.array_equal(got, want)
    dp.close()
