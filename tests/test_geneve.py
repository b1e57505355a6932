"""Geneve tunnel mode: the option check of from_overlay compiled with ENCAP_GENEVE
(gf_overlay_classify_opts on a program loaded with GF_OVERLAY_F_GENEVE; bpf/bpf_overlay.c:54-67,
bpf/lib/geneve.h:46-60) and the tunnel metadata encap_and_redirect sets on the sending node
(gf_lxc_egress_tunnel_meta; bpf/lib/encap.h:30-81), up to a packet that leaves node A's
container and reaches handle_policy on node B, all on the device.

Expected values come from tests/geneve_model.py (the reference's option check around
tests/overlay_model.py's front) followed by OracleDP.ingress over the delivered subset, as
tests/test_overlay.py does for VXLAN, and from the hand-derived cases of
tests/golden/geneve_kats.json.  Ring records: TRACE_FROM_OVERLAY and the front's drops as
tests/netdev_model.py writes the pipeline front's; handle_policy's drop records by the layout of
bpf/lib/drop.h:38-107, their header tied to the oracle's on the CPU.
"""
import copy
import errno
import json
import os
import struct
import types

import numpy as np
import pytest

from cilium_amd import geneve, synth
from cilium_amd.synth import Packets
from oracle.scenario import OracleDP
from tests import ctoff_model as CM
from tests import geneve_model as GM
from tests import netdev_model as NM
from tests import overlay_model as OM
from tests.overlay_model import PIPE_OUT

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KAT_NOW = 5000
F_TRACE, F_GENEVE = 1, 2                                 # GF_OVERLAY_F_TRACE_NOTIFY, GF_OVERLAY_F_GENEVE
EG_OUT = np.dtype([("stage", "u1"), ("action", "u1"), ("reason", "u1"), ("ct_ret", "u1"), ("flags", "u1"),
                   ("eg_ct_ret", "u1"), ("proxy_port", "<u2"), ("ifindex_lo", "<u2"), ("slave", "<u2"),
                   ("rev_nat", "<u2"), ("eg_flags", "<u2"), ("tunnel_ip", "<u4"), ("lxc_id", "<u2"), ("pad", "<u2")])


# ---------------------------------------------------------------- KATs
def _kats():
    with open(os.path.join(GOLDEN, "geneve_kats.json")) as f:
        return json.load(f)["cases"]


def kat_scenario(flags=F_GENEVE):
    """The KATs as one batch over the endpoints of tests/test_overlay.py's kat_scenario (HOST_IFINDEX 3).
    Returns (scenario, cases, expected PIPE_OUT records, expected frames, opt [n,8], opt_len [n])."""
    cases = _kats()
    sc = synth.Scenario("geneve_kats", now=KAT_NOW, host_ifindex=3)
    mac = lambda s: np.frombuffer(bytes.fromhex(s), np.uint8)
    a6 = np.frombuffer(bytes.fromhex("f00d" + "00" * 13 + "01"), np.uint8)
    h6 = np.frombuffer(bytes.fromhex("f00d" + "00" * 13 + "fe"), np.uint8)
    keys = np.concatenate([synth.endpoint_keys4([synth.ip4("10.1.0.1"), synth.ip4("10.1.0.2"), synth.ip4("10.1.0.254")]),
                           synth.endpoint_keys6(np.stack([a6, h6]))])
    vals = synth.endpoint_infos(np.array([11, 12, 1, 11, 1]), np.zeros(5), np.array([3000, 3001, 0, 3000, 0]),
                                np.array([0, 0, 1, 0, 1]))
    for row, (m, nm) in {0: ("aa1111111111", "bb2222222222"), 1: ("aa3333333333", "bb4444444444"),
                         3: ("aa1111111111", "bb2222222222")}.items():
        vals[row, 16:22], vals[row, 24:30] = mac(m), mac(nm)
    sc.add_map(synth.MapSpec("cilium_lxc", synth.HASH, 20, 112, 1024, 0, keys, vals))
    sc.add_map(synth.MapSpec("ct4", synth.LRU_HASH, 14, 48, 4096, 0))
    sc.add_map(synth.MapSpec("ct6", synth.LRU_HASH, 40, 48, 4096, 0))
    for k, lid in enumerate((3000, 3001)):
        sc.add_map(synth.MapSpec(f"pol{k}", synth.HASH, 8, 24, 1024, 0, synth.policy_keys([300], [0], [0]),
                                 synth.policy_vals([0])))
        sc.lxc.append({"lxc_id": lid, "seclabel": 500 + k, "policy": f"pol{k}", "ct4": "ct4", "ct6": "ct6",
                       "flags": synth.LXC_PRODUCTION, "l4": []})
    sc.node = {"host_mac": bytes.fromhex("ce72a7038856"), "node_mac": bytes.fromhex("deadbeefc0de")}
    sc.overlay = {"lxc_map": "cilium_lxc", "flags": flags, "ingress_ifindex": 9}
    n, S = len(cases), 128
    frames, lens = np.zeros((n, S), np.uint8), np.zeros(n, np.uint32)
    want, wantf = np.zeros(n, PIPE_OUT), np.zeros((n, S), np.uint8)
    opt, ol = np.zeros((n, 8), np.uint8), np.zeros(n, np.uint8)
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
        opt[k] = np.frombuffer(bytes.fromhex(c["opt"]), np.uint8)
        ol[k] = c["opt_len"]
    tid = np.array([c["tunnel_id"] for c in cases], np.uint32)
    sc.batches.append(Packets(frames, lens, None, None, None, np.zeros(n, np.uint8), np.zeros(n, np.uint32), tid))
    return sc, cases, want, wantf, opt, ol


def model_run(pk, opt, ol, now, ref, model):
    """The model's front with the option check, then the oracle's handle_policy over the delivered
    subset in batch order.  Returns (records, front frames, front records, delivered indices, the
    delivered subset)."""
    rec, frames, dl, sub = model.front(pk, ref.parse(pk), opt, ol)
    ing = ref.ingress(sub, now) if sub.n else np.zeros(0, CM.ING_OUT)
    return OM.complete(rec, dl, ing), frames, rec, dl, sub


def test_kats_cover_the_issue_list():
    cases = _kats()
    names = [c["name"] for c in cases]
    assert len(names) == len(set(names)) and all(c["derivation"] for c in cases)
    assert set(names) >= {"v6_valid_opt8_delivered", "v6_valid_opt_non_local", "v6_no_opt_known_daddr", "v6_opt_len_68",
                          "v6_wrong_class", "v6_wrong_type", "v6_length_field_2", "v6_reserved_bits_length_1",
                          "v6_opt_len_2", "v6_opt_len_4", "v6_len50_no_opt", "v4_no_opt_delivered", "arp_garbage_opt",
                          "v6_host_bad_opt"}
    by = {c["name"]: c for c in cases}
    assert by["v6_no_opt_known_daddr"]["expect"]["reason"] == 148 and by["v6_opt_len_68"]["expect"]["reason"] == 148
    assert by["v6_len50_no_opt"]["expect"]["reason"] == 134 and by["v6_host_bad_opt"]["changed"] == {}
    assert by["v6_opt_len_2"]["opt"].startswith("ffff0101")     # the stale bytes past options_len are valid ones


def test_model_reproduces_every_kat():
    sc, cases, want, wantf, opt, ol = kat_scenario()
    got, frames, _, _, _ = model_run(sc.batches[0], opt, ol, sc.now, OracleDP(sc), GM.GeneveModel(sc))
    for k, c in enumerate(cases):
        assert got[k] == want[k], (c["name"], got[k], want[k])
        assert bytes(frames[k]) == bytes(wantf[k]), c["name"]


def test_ipv4_and_non_ip_ignore_their_options():
    """handle_ipv4 has no ENCAP_GENEVE block: whatever the option columns hold, IPv4 and non-IP
    frames end as the VXLAN model's."""
    sc, pk, opt, ol = fuzz_case(128, 8)
    cols = OracleDP(sc).parse(pk)
    m = cols["ethertype"] != 0x86DD
    sub = Packets(pk.frames[m], pk.lens[m], None, None, None, pk.tc_index[m], pk.flow_hash[m], pk.tunnel_id[m])
    c2 = {k: v[m] for k, v in cols.items()}
    r0, f0, d0, _ = OM.OverlayModel(sc).front(sub, c2)
    gm = GM.GeneveModel(sc)
    r1, f1, d1, _ = gm.front(sub, c2, opt[m], ol[m])
    assert m.sum() > 1000 and (r0 == r1).all() and not (f0 != f1).any() and np.array_equal(d0, d1) and not gm.gnv.any()


# ---------------------------------------------------------------- cilium_amd.geneve
def test_geneve_module_round_trip():
    want = bytes([0xff, 0xff, 0x1, 0x1, 0x0, 0x0, 0x1, 0x1e])   # bpf/lxc_config.h:35 GENEVE_OPTS
    tlvs, raw = geneve.encode("ffff;1;4;0000011e\n")
    assert raw == want and tlvs == [geneve.GeneveTlv(0xffff, 1, 4, bytes.fromhex("0000011e"))]
    assert geneve.encode("0xffff;0x1;4;0000011e")[1] == want     # as writeGeneve passes them to WriteOpts
    assert geneve.decode(want) == tlvs
    assert geneve.encode(geneve.lines(geneve.decode(want)))[1] == want
    assert geneve.endpoint_opts(0x11e) == want
    two = geneve.encode("0xffff;1;4;0000011e\n0x0102;0x80;8;0011223344556677\n")
    assert two[1] == want + bytes([1, 2, 0x80, 2]) + bytes.fromhex("0011223344556677")
    assert geneve.decode(two[1]) == two[0]
    assert geneve.decode(bytes([0xff, 0xff, 1, 0xe1, 0, 0, 1, 0x1e])) == tlvs   # reserved bits ignored


@pytest.mark.parametrize("line,why", [("0xffff;1;128;" + "00" * 128, "sz > 124"), ("0xffff;1;6;000000000000", "sz % 4"),
                                      ("0xffff;1;8;0000011e", "len(data)")])
def test_geneve_module_rejects_validate_failures(line, why):
    c, t, sz, hx = line.split(";")
    assert not geneve.validate(geneve.GeneveTlv(int(c, 0), int(t), int(sz), bytes.fromhex(hx))), why
    with pytest.raises(ValueError):
        geneve.encode(line)
    assert geneve.validate(geneve.GeneveTlv(0xffff, 1, 124, bytes(124)))


@pytest.mark.parametrize("identity", [0, 1, 0x11e, 0xffffffff])
def test_transmit_bytes_pass_the_receive_check(identity):
    tx = GM.tx_opts(identity)
    assert tx == geneve.endpoint_opts(identity) and len(tx) == 8
    ret, buf = GM.get_tunnel_opt(tx, len(tx))
    assert ret == 8 and GM.parse_geneve_options(buf) == (0, identity)
    assert GM.rx_check(0x86DD, 74, tx, 8) == 0
    assert GM.rx_check(0x86DD, 74, tx, 0) == -148 and GM.rx_check(0x86DD, 74, tx, 3) == -149


# ---------------------------------------------------------------- fuzz batch
_FUZZ = {}


def gen_opts(rng, n, opt_stride, valid=False):
    """Option columns: valid seclabel options (any reserved bits, options_len 4..64), no options,
    options_len past the buffer, options_len 1..3 over valid bytes, and a wrong class / type /
    length; the bytes behind the first four are random."""
    opt = rng.integers(0, 256, (n, opt_stride)).astype(np.uint8)
    opt[:, 0:3] = (0xff, 0xff, 0x01)
    opt[:, 3] = 1 | (rng.integers(0, 8, n) << 5)
    ol = (4 * rng.integers(1, 17, n)).astype(np.uint8)
    if valid:
        return opt, ol
    k = rng.random(n)
    ol[k < 0.10] = 0
    m = (k >= 0.10) & (k < 0.14)
    ol[m] = rng.integers(65, 256, int(m.sum()))
    m = (k >= 0.14) & (k < 0.18)
    ol[m] = rng.integers(1, 4, int(m.sum()))
    m = np.nonzero((k >= 0.18) & (k < 0.30))[0]
    which = rng.integers(0, 4, len(m))
    opt[m[which == 0], 0] = rng.integers(0, 255, int((which == 0).sum()))
    opt[m[which == 1], 1] = rng.integers(0, 255, int((which == 1).sum()))
    opt[m[which == 2], 2] = rng.choice(np.array([0, 2, 3, 0x81, 0xff], np.uint8), int((which == 2).sum()))
    opt[m[which == 3], 3] = rng.choice(np.array([0, 2, 3, 0x1f, 0xe0, 0xe2], np.uint8), int((which == 3).sum()))
    return opt, ol


def fuzz_case(stride, opt_stride, flags=F_GENEVE):
    """About 4k overlay_fuzz frames cut to `stride` with option columns of `opt_stride`."""
    key = (stride, opt_stride)
    if key not in _FUZZ:
        sc = synth.overlay_fuzz(seed=11, n_packets=4096, n_batches=1)
        pk = sc.batches[0]
        pk = Packets(np.ascontiguousarray(pk.frames[:, :stride]), pk.lens, None, None, None, pk.tc_index, pk.flow_hash,
                     pk.tunnel_id)
        sc.batches[0] = pk
        opt, ol = gen_opts(np.random.default_rng(stride * 1000 + opt_stride), pk.n, opt_stride)
        _FUZZ[key] = (sc, pk, opt, ol)
    sc, pk, opt, ol = _FUZZ[key]
    sc = copy.copy(sc)
    sc.overlay = dict(sc.overlay, flags=flags)
    return sc, pk, opt, ol


def fuzz_classes(sc, pk, opt, ol, want, gnv):
    v4, v6 = pk.frames[:, 12] == 0x08, (pk.frames[:, 12] == 0x86) & (pk.frames[:, 13] == 0xDD)
    s4, s6 = want["stage"] == 4, want["stage"] == 6
    bad_opt = np.array([GM.rx_check(0x86DD, 74, opt[i], int(ol[i])) != 0 for i in range(pk.n)])
    return {"no_tunnel_opt": s6 & (want["reason"] == 148), "invalid_geneve": s6 & (want["reason"] == 149),
            "v6_delivered": v6 & s4,
            "v6_to_host": v6 & s6 & (want["action"] == 7) & (want["ifindex_lo"] == sc.host_ifindex) & (want["flags"] & 0x20 == 0),
            "v6_non_local_valid_opt": v6 & s6 & (want["reason"] == 151) & ~bad_opt,
            "v4_bad_opt": v4 & (pk.frames[:, 13] == 0) & bad_opt}


@pytest.mark.parametrize("stride,opt_stride", [(128, 8), (256, 64)])
def test_fuzz_batch_is_not_thin(stride, opt_stride):
    sc, pk, opt, ol = fuzz_case(stride, opt_stride)
    model = GM.GeneveModel(sc)
    want, _, _, _, _ = model_run(pk, opt, ol, sc.now, OracleDP(sc), model)
    for name, m in fuzz_classes(sc, pk, opt, ol, want, model.gnv).items():
        assert m.sum() >= 32, (name, int(m.sum()))
    assert ((model.gnv < 0) == np.isin(want["reason"], (148, 149))).all()


def policy_drop_event(sc, ifindex, o, ln, tid, frame, fh):
    """handle_policy's drop record (drop.h:47-107): source = LXC_ID, src_label = the low 16 bits of
    the source identity, dst_label = SECLABEL, dst_id = LXC_ID, ifindex = the endpoint entry's
    (cb[CB_IFINDEX] as ipv{4,6}_local_delivery set it)."""
    e = {x["lxc_id"]: x for x in sc.lxc}[int(o["lxc_id"])]
    return NM.event(1 | (int(o["reason"]) << 8) | (e["lxc_id"] << 16), ln, tid & 0xffff, e["seclabel"], e["lxc_id"],
                    ifindex, frame, fh)


def ipv6_policy_zero_rev_nat(frame, length, nexthdr, l4_off):
    """ipv6_policy's first write (bpf_lxc.c:775-792), which precedes conntrack and the policy
    check and so shows in the payload of every drop record it sends: rev_nat_index =
    daddr.s6_addr32[3] & 0xFFFF; when non-zero those two bytes are zeroed and the L4 checksum
    corrected by csum_diff(&rev_nat_index, 4, &zero, 4, 0) (DROP_CSUM_L4 after the store where the
    field lies outside the frame)."""
    f = frame.copy()
    rn = int(f[50]) | (int(f[51]) << 8)
    if rn:
        f[50] = f[51] = 0
        co = CM.csum_offset(nexthdr)
        if co and CM.l4_csum_replace_ok(l4_off + co, length):
            CM.l4_csum_replace_by_diff(f, min(length, len(f)), l4_off + co, CM.csum_add(0xffffffff ^ rn, 0),
                                       nexthdr == CM.IPPROTO_UDP)
    return f


def expected_events(sc, pk, want, frames, dl, sub):
    """Per packet: TRACE_FROM_OVERLAY (bpf_overlay.c:174: the frame as received, ifindex =
    ingress_ifindex) when the program has TRACE_NOTIFY, then the drop record of a SHOT: the front's
    (send_drop_notify_error: zeros) or handle_policy's.  No endpoint program traces here."""
    ifx = dict(zip(dl.tolist(), sub.ifindex.tolist()))
    cols = OracleDP(sc).parse(pk)
    progs = {e["lxc_id"]: e for e in sc.lxc}
    out = []
    for i in range(pk.n):
        o, ln, ev = want[i], int(pk.lens[i]), []
        fh = 0 if pk.flow_hash is None else int(pk.flow_hash[i])
        if sc.overlay["flags"] & F_TRACE:
            ev.append(NM.event(4 | (9 << 8), ln, 0, 0, 0, sc.overlay["ingress_ifindex"], pk.frames[i], fh))
        if o["action"] == OM.TC_ACT_SHOT:
            if o["stage"] == OM.STAGE_OVERLAY:
                ev.append(NM.event(1 | (int(o["reason"]) << 8), ln, 0, 0, 0, 0, frames[i], fh))
            else:
                fr = frames[i]
                drop_all = progs[int(o["lxc_id"])]["flags"] & synth.LXC_DROP_ALL   # bpf_lxc.c:986-989: ipv6_policy never runs
                if cols["ethertype"][i] == 0x86DD and not drop_all:
                    fr = ipv6_policy_zero_rev_nat(fr, ln, int(cols["proto"][i]), int(cols["l4_off"][i]))
                ev.append(policy_drop_event(sc, ifx[i], o, ln, int(pk.tunnel_id[i]), fr, fh))
        out.append(ev)
    return out


def test_policy_drop_header_is_the_oracles():
    """Ties the hand-written handle_policy drop record to the oracle's (which has no frames, so
    len_cap and the payload are left out)."""
    sc, pk, opt, ol = fuzz_case(128, 8)
    ref, model = OracleDP(sc), GM.GeneveModel(sc)
    want, frames, _, dl, sub = model_run(pk, opt, ol, sc.now, ref, model)
    ing = np.zeros(len(dl), CM.ING_OUT)
    for name in ("action", "reason", "ct_ret", "proxy_port", "ifindex_lo"):
        ing[name] = want[name][dl]
    oe = ref.ingress_events(sub, ing)
    ev = expected_events(sc, pk, want, frames, dl, sub)
    mine = np.stack([ev[i][-1] for i in dl if want["action"][i] == 2])
    assert len(mine) == len(oe) > 100
    hdr = lambda e: np.delete(e[:, :32], np.s_[12:16], axis=1)
    assert np.array_equal(hdr(mine), hdr(oe))
    # the payload: the oracle's from_netdev over the same frames (no XDP / LB, one identity no policy
    # map holds) delivers them as from_overlay does and carries the frame in handle_policy's drop record
    import oracle.oracle as O
    idx = np.array([i for i in dl if want["action"][i] == 2])
    nd = copy.copy(sc)
    nd.xdp = nd.lb = None
    nd.netdev = dict(sc.netdev, flags=1, fixed_secctx=999999, ingress_ifindex=9)
    with O.TraceSink(len(idx)) as ts:
        ro, _, _ = OracleDP(nd).pipeline(Packets(pk.frames[idx], pk.lens[idx], None, None, None, pk.tc_index[idx],
                                                 pk.flow_hash[idx]), sc.now)
    both = (ro["stage"] == 4) & (ro["action"] == 2)
    assert both.sum() > len(idx) * 0.9 and (both & (pk.frames[idx, 12] == 0x86)).sum() >= 32
    for j in np.nonzero(both)[0]:
        assert np.array_equal(ts.ev[j, ts.cnt[j] - 1, 32:], mine[j, 32:]), (j, idx[j])


# ---------------------------------------------------------------- two nodes
def two_node_scenarios():
    """Node A: egress_fuzz's endpoints and the frames of one batch that its from-container program
    encapsulates (the tunnel map covers the destination, cilium_lxc does not hold it) with a TTL /
    hop limit node B can still decrement, among frames that take other paths.  Node B: a cilium_lxc
    holding every destination of those frames, four endpoints whose policy maps allow every second
    sender identity.  Returns (scA, scB, oracle egress records of A, oracle frames of A)."""
    scA = synth.egress_fuzz(seed=5, n_packets=3000, n_batches=1)
    pk = scA.batches[0]
    far6 = np.nonzero((pk.frames[:, 12] == 0x86) & (np.arange(pk.n) % 2 == 0))[0]   # half of the IPv6 frames to the
    pk.frames[far6, 38:50] = scA.meta["rem6"][7][:12]                               # prefix the tunnel map holds
    ro, rs = OracleDP(scA).egress(pk, scA.now)
    enc = ro["eg_flags"] & GM.EG_F_ENCAP != 0
    alive = np.where(rs[:, 12] == 0x08, rs[:, 22] > 1, rs[:, 21] > 1)
    keep = (enc & alive) | (~enc & (np.arange(pk.n) % 4 == 0))
    pk = Packets(pk.frames[keep], pk.lens[keep], None, None, pk.lxc_id[keep], None, pk.flow_hash[keep])
    scA.batches = [pk]
    ro, rs = OracleDP(scA).egress(pk, scA.now)
    enc = ro["eg_flags"] & GM.EG_F_ENCAP != 0
    v4 = rs[:, 12] == 0x08
    k4 = np.unique(rs[enc & v4, 30:34], axis=0)
    k6 = np.unique(rs[enc & ~v4, 38:54], axis=0)
    keys = np.zeros((len(k4) + len(k6), 20), np.uint8)
    keys[:len(k4), 0:4], keys[:len(k4), 16] = k4, 1
    keys[len(k4):, 0:16], keys[len(k4):, 16] = k6, 2
    ep = np.arange(len(keys)) % 4
    vals = synth.endpoint_infos(11 + ep, np.zeros(len(keys)), 3000 + ep, np.zeros(len(keys)))
    vals[:, 16:22] = np.frombuffer(bytes.fromhex("aa1111111111"), np.uint8)
    vals[:, 21] = ep
    vals[:, 24:30] = np.frombuffer(bytes.fromhex("bb2222222222"), np.uint8)
    scB = synth.Scenario("nodeB", now=scA.now, host_ifindex=3)
    scB.add_map(synth.MapSpec("cilium_lxc", synth.HASH, 20, 112, 4096, 0, keys, vals))
    scB.add_map(synth.MapSpec("ct4", synth.LRU_HASH, 14, 48, 65536, 0))
    scB.add_map(synth.MapSpec("ct6", synth.LRU_HASH, 40, 48, 65536, 0))
    senders = sorted({e["seclabel"] for e in scA.lxc})
    allow = senders[::2]
    for k in range(4):
        scB.add_map(synth.MapSpec(f"pol{k}", synth.HASH, 8, 24, 1024, 0,
                                  synth.policy_keys(allow, [0] * len(allow), [0] * len(allow)),
                                  synth.policy_vals([0] * len(allow))))
        scB.lxc.append({"lxc_id": 3000 + k, "seclabel": 700 + k, "policy": f"pol{k}", "ct4": "ct4", "ct6": "ct6",
                        "flags": synth.LXC_PRODUCTION, "l4": []})
    scB.node = {"host_mac": bytes.fromhex("ce72a7038856"), "node_mac": bytes.fromhex("deadbeefc0de")}
    scB.overlay = {"lxc_map": "cilium_lxc", "flags": F_GENEVE, "ingress_ifindex": 9}
    return scA, scB, ro, rs


def corrupt(pkB, opt):
    """One byte of the last IPv6 packet's option (its type) and of one IPv4 packet's.  The last IPv6
    packet: no later packet can meet conntrack state it would have left."""
    v6 = np.nonzero(pkB.frames[:, 12] == 0x86)[0]
    v4 = np.nonzero(pkB.frames[:, 12] == 0x08)[0]
    j6, j4 = int(v6[-1]), int(v4[len(v4) // 2])
    bad = opt.copy()
    bad[j6, 2] ^= 0x02
    bad[j4, 0] ^= 0x80
    return bad, j6, j4


def test_two_node_loop_on_the_models():
    """The loop with the oracle's egress records in place of the device's: what the GPU test relies
    on holds by the model and the reference alone."""
    scA, scB, ro, rs = two_node_scenarios()
    pkA = scA.batches[0]
    tid, opt, ol = GM.tx_meta(scA, pkA.lxc_id, ro)
    enc = ro["eg_flags"] & GM.EG_F_ENCAP != 0
    v6 = enc & (rs[:, 12] == 0x86)
    assert (enc & ~v6).sum() >= 100 and v6.sum() >= 32 and (~enc).sum() >= 100
    assert not tid[~enc].any() and not opt[~enc].any() and not ol[~enc].any() and (ol[enc] == 8).all()
    sec = {e["lxc_id"]: e["seclabel"] for e in scA.lxc}
    assert all(tid[i] == sec[int(pkA.lxc_id[i])] for i in np.nonzero(enc)[0])
    pkB = Packets(rs[enc], pkA.lens[enc], None, None, None, None, None, tid[enc])
    want, _, front, dl, sub = model_run(pkB, opt[enc], ol[enc], scB.now, OracleDP(scB), GM.GeneveModel(scB))
    assert (front["stage"] == 4).all() and np.array_equal(sub.src_identity, tid[enc])
    deny = (want["action"] == 2) & (want["reason"] == 133)
    assert deny.sum() >= 32 and (want["action"] != 2).sum() >= 32
    allow = set(sorted(set(sec.values()))[::2])
    assert all((int(t) in allow) != bool(d) for t, d in zip(tid[enc], deny) )
    bad, j6, j4 = corrupt(pkB, opt[enc])
    w2, _, _, _, _ = model_run(pkB, bad, ol[enc], scB.now, OracleDP(scB), GM.GeneveModel(scB))
    diff = np.nonzero(w2 != want)[0]
    assert diff.tolist() == [j6] and (w2[j6]["stage"], w2[j6]["action"], w2[j6]["reason"]) == (6, 2, 149)


# ---------------------------------------------------------------- error returns without a device
def test_geneve_program_is_refused_by_plain_classify():
    import ctypes as C
    from cilium_amd import bpf
    from cilium_amd._lib import lib, gf_overlay_cfg, gf_overlay_batch, gf_tunnel_opts
    lxc = bpf.CreateMap(synth.HASH, 20, 112, 64, 0)
    arr = lib.gf_policy_array_create()
    try:
        gnv = lib.gf_overlay_load(C.byref(gf_overlay_cfg(lxc, F_GENEVE, 9, arr)))
        vx = lib.gf_overlay_load(C.byref(gf_overlay_cfg(lxc, 0, 9, arr)))
        assert gnv > 0 and vx > 0
        b, to = gf_overlay_batch(), gf_tunnel_opts()
        assert lib.gf_overlay_classify(gnv, C.byref(b), 0, None, None, None) == -errno.EINVAL
        assert lib.gf_overlay_classify_opts(gnv, C.byref(b), C.byref(to), 0, None, None, None) == 0      # n == 0
        assert lib.gf_overlay_classify_opts(vx, C.byref(b), None, 0, None, None, None) == 0
        assert lib.gf_overlay_classify_opts(lxc, C.byref(b), None, 0, None, None, None) == -errno.EBADF
        assert lib.gf_overlay_classify_opts(gnv, None, C.byref(to), 0, None, None, None) == -errno.EFAULT
        assert lib.gf_lxc_egress_tunnel_meta(lxc, None, None, 0, None, None, None, None) == -errno.EBADF
        assert lib.gf_lxc_egress_tunnel_meta(arr, None, None, 0, None, None, None, None) == 0
        assert lib.gf_lxc_egress_tunnel_meta(arr, None, None, 4, None, None, None, None) == -errno.EFAULT
        for h in (gnv, vx):
            bpf.ObjClose(h)
    finally:
        for h in (arr, lxc):
            bpf.ObjClose(h)


# ---------------------------------------------------------------- GPU
torch = pytest.importorskip("torch")


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(0)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _gpu_overlay(dp, pk, now, opt=None, ol=None, snap_out=True):
    from cilium_amd.datapath import DeviceBatch, to_numpy
    b = DeviceBatch(pk, parse=False)
    out, snap = dp.overlay(b, now, snap_out=snap_out, opt=None if opt is None else _dev(opt),
                           opt_len=None if ol is None else _dev(ol))
    torch.cuda.synchronize()
    return to_numpy(out, PIPE_OUT), None if snap is None else snap.cpu().numpy()


def _same(got, want, what):
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, f"{what}: {len(bad)} records differ, first {bad[:1]}: {got[bad[:1]]} != {want[bad[:1]]}"


def _frames_cmp(pk, want):
    """Packets whose frame handle_policy does not write (tests/test_overlay.py's module docstring)."""
    return (want["stage"] == 6) | ((pk.frames[:, 12] == 0x08) & (want["flags"] & 1 == 0) & (want["action"] != 2) &
                                   (want["ct_ret"] < 2))


def _ring(cap=16384):
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


def _maps_same(dp, ref, sc, what=""):
    for name in ["ct4", "ct6", "cilium_proxy4", "cilium_proxy6"] + [e["policy"] for e in sc.lxc]:
        if name in sc.maps:
            assert dp.dump_map(name) == ref.dump(name), (what, name)


@pytest.mark.gpu
def test_gpu_kats():
    """The KATs through gf_overlay_classify_opts: records, snap_out, every map against the model +
    the oracle's handle_policy."""
    _gpu()
    from cilium_amd.datapath import Datapath
    sc, cases, want, wantf, opt, ol = kat_scenario()
    dp, ref = Datapath(sc, pin_prefix=None), OracleDP(sc)
    try:
        got, snap = _gpu_overlay(dp, sc.batches[0], sc.now, opt, ol)
        wm, _, _, _, _ = model_run(sc.batches[0], opt, ol, sc.now, ref, GM.GeneveModel(sc))
        for k, c in enumerate(cases):
            assert got[k] == want[k] == wm[k], (c["name"], got[k], want[k])
            assert bytes(snap[k]) == bytes(wantf[k]), c["name"]
        _maps_same(dp, ref, sc)
    finally:
        dp.close()


@pytest.mark.gpu
@pytest.mark.parametrize("stride,opt_stride,events", [(128, 8, None), (256, 64, "trace"), (128, 64, "ring"), (256, 8, None)])
def test_gpu_fuzz(stride, opt_stride, events):
    """The fuzz batch against the model + OracleDP.ingress: records, frames (dropped rows equal the
    input), every CT / policy / proxy map; with the event ring the ring against the model's
    per-packet lists, in one variant with GF_OVERLAY_F_TRACE_NOTIFY."""
    _gpu()
    import ctypes as C
    from cilium_amd._lib import lib
    from cilium_amd.datapath import Datapath
    sc, pk, opt, ol = fuzz_case(stride, opt_stride, F_GENEVE | (F_TRACE if events == "trace" else 0))
    ref, model = OracleDP(sc), GM.GeneveModel(sc)
    want, frames, _, dl, sub = model_run(pk, opt, ol, sc.now, ref, model)
    for name, m in fuzz_classes(sc, pk, opt, ol, want, model.gnv).items():
        assert m.sum() >= 32, (name, int(m.sum()))
    dp = Datapath(sc, pin_prefix=None)
    recs, cnt, ring = _ring()
    if events:
        assert lib.gf_set_event_ring(C.byref(ring)) == 0
    try:
        got, snap = _gpu_overlay(dp, pk, sc.now, opt, ol)
        _same(got, want, "records")
        cmp = _frames_cmp(pk, want)
        assert not (snap[cmp] != frames[cmp]).any(), "frames"
        dropped = np.isin(want["reason"], (148, 149))
        assert dropped.sum() >= 64 and not (snap[dropped] != pk.frames[dropped]).any()
        _maps_same(dp, ref, sc)
        if events:
            ev = expected_events(sc, pk, want, frames, dl, sub)
            exp = np.stack([r for e in ev for r in e])
            assert (exp[:, 0] == 4).sum() == (pk.n if events == "trace" else 0) and (exp[:, 1] == 148).sum() >= 32
            _ring_check(recs, cnt, exp, events)
    finally:
        lib.gf_set_event_ring(None)
        dp.close()


@pytest.mark.gpu
@pytest.mark.parametrize("stride", [128, 256])
def test_gpu_block_boundary(stride):
    """Batches of 1, 255, 256 and 257 packets (one block, and a second one of a single lane at both
    tile sizes), with and without snap_out, one after the other on one datapath and one oracle."""
    _gpu()
    from cilium_amd.datapath import Datapath
    sc, full, opt, ol = fuzz_case(stride, 8)
    dp, ref, model = Datapath(sc, pin_prefix=None), OracleDP(sc), GM.GeneveModel(sc)
    try:
        for n in (1, 255, 256, 257):
            pk = full.slice(4096 - n, 4096)
            o, l = opt[4096 - n:], ol[4096 - n:]
            for snap_out in (True, False):
                got, snap = _gpu_overlay(dp, pk, sc.now, o, l, snap_out=snap_out)
                want, frames, _, _, _ = model_run(pk, o, l, sc.now, ref, model)
                _same(got, want, f"n {n} snap_out {snap_out}")
                if snap_out:
                    cmp = _frames_cmp(pk, want)
                    assert not (snap[cmp] != frames[cmp]).any(), n
            assert n == 1 or np.isin(want["reason"], (148, 149)).any()
    finally:
        dp.close()


def _run_all(sc, pk, call):
    """One datapath over the scenario with the event ring on: returns (records, frames, map dumps,
    ring records)."""
    import ctypes as C
    from cilium_amd._lib import lib
    from cilium_amd.datapath import Datapath
    recs, cnt, ring = _ring()
    dp = Datapath(sc, pin_prefix=None)
    assert lib.gf_set_event_ring(C.byref(ring)) == 0
    try:
        got, snap = call(dp)
        names = ["ct4", "ct6", "cilium_proxy4", "cilium_proxy6"] + [e["policy"] for e in sc.lxc]
        dumps = {name: dp.dump_map(name) for name in names}
        ev = recs[:int(cnt.item())].cpu().numpy()
    finally:
        lib.gf_set_event_ring(None)
        dp.close()
    return got, snap, dumps, ev


@pytest.mark.gpu
def test_gpu_valid_options_equal_vxlan():
    """All-valid options under a Geneve program give records, frames, maps and events byte-equal to
    a VXLAN program through gf_overlay_classify."""
    _gpu()
    scg, pk, _, _ = fuzz_case(256, 64, F_GENEVE | F_TRACE)
    scv, _, _, _ = fuzz_case(256, 64, F_TRACE)
    opt, ol = gen_opts(np.random.default_rng(5), pk.n, 64, valid=True)
    g = _run_all(scg, pk, lambda dp: _gpu_overlay(dp, pk, scg.now, opt, ol))
    v = _run_all(scv, pk, lambda dp: _gpu_overlay(dp, pk, scv.now))
    assert (g[0]["stage"] == 4).sum() > 1000 and len(g[3]) > pk.n
    _same(g[0], v[0], "records")
    assert np.array_equal(g[1], v[1]) and g[2] == v[2] and np.array_equal(g[3], v[3])


@pytest.mark.gpu
def test_gpu_vxlan_program_ignores_options():
    """A VXLAN program through gf_overlay_classify_opts with garbage options (and with opts NULL)
    equals plain gf_overlay_classify."""
    _gpu()
    import ctypes as C
    from cilium_amd._lib import lib, gf_frames, gf_overlay_batch
    from cilium_amd.datapath import Datapath, DeviceBatch, to_numpy
    sc, pk, opt, ol = fuzz_case(128, 8, F_TRACE)
    junk = np.random.default_rng(9).integers(0, 256, opt.shape).astype(np.uint8)
    a = _run_all(sc, pk, lambda dp: _gpu_overlay(dp, pk, sc.now, junk, ol))
    b = _run_all(sc, pk, lambda dp: _gpu_overlay(dp, pk, sc.now))
    _same(a[0], b[0], "records")
    assert np.array_equal(a[1], b[1]) and a[2] == b[2] and np.array_equal(a[3], b[3])
    assert not np.isin(a[0]["reason"], (148, 149)).any()
    dp = Datapath(sc, pin_prefix=None)
    try:
        d = DeviceBatch(pk, parse=False)
        out = torch.empty((d.n, 24), dtype=torch.uint8, device="cuda")
        ob = gf_overlay_batch(gf_frames(d.n, 128, d.frames.data_ptr(), d.len.data_ptr()), d.tunnel_id.data_ptr(),
                              d.tc_index.data_ptr(), d.flow_hash.data_ptr())
        assert lib.gf_overlay_classify_opts(dp.ovl, C.byref(ob), None, sc.now, out.data_ptr(), None, None) == 0
        torch.cuda.synchronize()
        _same(to_numpy(out, PIPE_OUT), b[0], "opts NULL")
    finally:
        dp.close()


@pytest.mark.gpu
def test_gpu_refusals_launch_nothing():
    """Every refusal precedes any launch: outputs pre-filled with a poison byte stay poisoned."""
    _gpu()
    import ctypes as C
    from cilium_amd._lib import lib, gf_frames, gf_overlay_batch, gf_tunnel_opts
    from cilium_amd.datapath import Datapath, DeviceBatch
    sc, cases, want, wantf, opt, ol = kat_scenario()
    dp = Datapath(sc, pin_prefix=None)
    try:
        b = DeviceBatch(sc.batches[0], parse=False)
        out = torch.full((b.n, 24), 0xA5, dtype=torch.uint8, device="cuda")
        snap = torch.full((b.n, 128), 0xA5, dtype=torch.uint8, device="cuda")
        wide = torch.zeros((b.n, 72), dtype=torch.uint8, device="cuda")
        dopt, dol = _dev(opt), _dev(ol)
        ob = gf_overlay_batch(gf_frames(b.n, 128, b.frames.data_ptr(), b.len.data_ptr()), b.tunnel_id.data_ptr(), None, None)

        def opts(to):
            return lib.gf_overlay_classify_opts(dp.ovl, C.byref(ob), None if to is None else C.byref(to), sc.now,
                                                out.data_ptr(), snap.data_ptr(), None)

        assert lib.gf_overlay_classify(dp.ovl, C.byref(ob), sc.now, out.data_ptr(), snap.data_ptr(), None) == -errno.EINVAL
        assert opts(None) == -errno.EFAULT
        assert opts(gf_tunnel_opts(None, 8, dol.data_ptr())) == -errno.EFAULT
        assert opts(gf_tunnel_opts(dopt.data_ptr(), 8, None)) == -errno.EFAULT
        for stride in (0, 2, 6, 68, 72):
            assert opts(gf_tunnel_opts(wide.data_ptr(), stride, dol.data_ptr())) == -errno.EINVAL, stride
        assert opts(gf_tunnel_opts(wide.data_ptr() + 2, 8, dol.data_ptr())) == -errno.EINVAL     # opt not 4-byte aligned
        torch.cuda.synchronize()
        assert bool((out == 0xA5).all()) and bool((snap == 0xA5).all())
        assert opts(gf_tunnel_opts(dopt.data_ptr(), 8, dol.data_ptr())) == 0
        torch.cuda.synchronize()
        assert not bool((out == 0xA5).all())
        # gf_lxc_egress_tunnel_meta
        tid = torch.full((b.n,), 0x25252525, dtype=torch.int32, device="cuda")
        mo = torch.full((b.n + 1, 8), 0xA5, dtype=torch.uint8, device="cuda")
        ml = torch.full((b.n,), 0xA5, dtype=torch.uint8, device="cuda")
        lid = torch.zeros(b.n, dtype=torch.int16, device="cuda")
        rec = torch.zeros((b.n, 24), dtype=torch.uint8, device="cuda")
        meta = lambda arr, l, r, t, o, n: lib.gf_lxc_egress_tunnel_meta(arr, l, r, b.n, t, o, n, None)
        p = lambda t: t.data_ptr()
        assert meta(dp.ovl, p(lid), p(rec), p(tid), p(mo), p(ml)) == -errno.EBADF
        for k in range(5):
            a = [p(lid), p(rec), p(tid), p(mo), p(ml)]
            a[k] = None
            assert meta(dp.policy_array, *a) == -errno.EFAULT
        assert meta(dp.policy_array, p(lid), p(rec), p(tid), p(mo) + 2, p(ml)) == -errno.EINVAL
        torch.cuda.synchronize()
        assert bool((tid == 0x25252525).all()) and bool((mo == 0xA5).all()) and bool((ml == 0xA5).all())
    finally:
        dp.close()


@pytest.mark.gpu
def test_gpu_egress_tunnel_meta():
    """gf_lxc_egress_tunnel_meta on the records of an egress fuzz batch with tunnel traffic: all three
    columns against the model; rows without GF_EG_F_ENCAP are zero."""
    _gpu()
    from cilium_amd.datapath import Datapath, DeviceBatch, to_numpy
    sc = synth.egress_fuzz(seed=5, n_packets=4001, n_batches=1)
    pk = sc.batches[0]
    dp, ref = Datapath(sc, pin_prefix=None), OracleDP(sc)
    try:
        b = DeviceBatch(pk, parse=False)
        out, _ = dp.egress(b, sc.now)
        tid, opt, ol = dp.egress_tunnel_meta(b.lxc_id, out)
        torch.cuda.synchronize()
        got = to_numpy(out, EG_OUT)
        ro, _ = ref.egress(pk, sc.now)
        _same(got, ro, "egress records")
        wt, wo, wl = GM.tx_meta(sc, pk.lxc_id, ro)
        enc = ro["eg_flags"] & GM.EG_F_ENCAP != 0
        assert enc.sum() >= 200 and (enc & (ro["eg_flags"] & 0x1000 != 0)).sum() >= 16 and len(set(wt[enc].tolist())) >= 8
        tid, opt, ol = tid.cpu().numpy().view(np.uint32), opt.cpu().numpy(), ol.cpu().numpy()
        assert np.array_equal(tid, wt) and np.array_equal(opt, wo) and np.array_equal(ol, wl)
        assert not tid[~enc].any() and not opt[~enc].any() and not ol[~enc].any()
    finally:
        dp.close()


@pytest.mark.gpu
def test_gpu_two_node_loop():
    """Node A's from-container program, gf_lxc_egress_tunnel_meta, the GF_EG_F_ENCAP rows compacted
    on the device, node B's Geneve from-overlay program and handle_policy: against the per-packet
    oracle run of B's handle_policy with src_label = the sender's seclabel."""
    _gpu()
    from cilium_amd.datapath import Datapath, DeviceBatch, to_numpy
    scA, scB, ro, rs = two_node_scenarios()
    pkA = scA.batches[0]
    dpA = Datapath(scA, pin_prefix=None)
    dpB = dpB2 = None
    try:
        bA = DeviceBatch(pkA, parse=False)
        out, snap = dpA.egress(bA, scA.now)
        tid, opt, ol = dpA.egress_tunnel_meta(bA.lxc_id, out)
        ef = out[:, 14].to(torch.int32) | (out[:, 15].to(torch.int32) << 8)      # gf_egress_out.eg_flags
        idx = ((ef & GM.EG_F_ENCAP) != 0).nonzero().squeeze(1)
        bB = types.SimpleNamespace(n=int(idx.numel()), device="cuda", frames=snap[idx].contiguous(), len=bA.len[idx].contiguous(),
                                   tunnel_id=tid[idx].contiguous(), tc_index=None, flow_hash=None)
        optB, olB = opt[idx].contiguous(), ol[idx].contiguous()
        torch.cuda.synchronize()
        # the device's node-A output is the oracle's
        enc = ro["eg_flags"] & GM.EG_F_ENCAP != 0
        _same(to_numpy(out, EG_OUT), ro, "node A records")
        wt, wo, wl = GM.tx_meta(scA, pkA.lxc_id, ro)
        pkB = Packets(bB.frames.cpu().numpy(), bB.len.cpu().numpy().view(np.uint32), None, None, None, None, None,
                      bB.tunnel_id.cpu().numpy().view(np.uint32))
        assert np.array_equal(pkB.frames, rs[enc]) and np.array_equal(pkB.tunnel_id, wt[enc])
        assert np.array_equal(optB.cpu().numpy(), wo[enc]) and np.array_equal(olB.cpu().numpy(), wl[enc])
        # node B
        dpB = Datapath(scB, pin_prefix=None)
        refB, model = OracleDP(scB), GM.GeneveModel(scB)
        o1, s1 = dpB.overlay(bB, scB.now, opt=optB, opt_len=olB)
        torch.cuda.synchronize()
        got = to_numpy(o1, PIPE_OUT).copy()
        want, frames, front, dl, sub = model_run(pkB, wo[enc], wl[enc], scB.now, refB, model)
        assert (front["stage"] == 4).all() and np.array_equal(sub.src_identity, wt[enc])
        _same(got, want, "node B records")
        deny = (want["action"] == 2) & (want["reason"] == 133)
        assert deny.sum() >= 32 and (want["action"] != 2).sum() >= 32
        cmp = _frames_cmp(pkB, want)
        assert not (s1.cpu().numpy()[cmp] != frames[cmp]).any()
        _maps_same(dpB, refB, scB)
        dpB.close()
        dpB = None
        # one corrupted byte in one IPv6 packet's option and in one IPv4 packet's, on a fresh node B
        bad, j6, j4 = corrupt(pkB, wo[enc])
        dpB2 = Datapath(scB, pin_prefix=None)
        o2, _ = dpB2.overlay(bB, scB.now, opt=_dev(bad), opt_len=olB)
        torch.cuda.synchronize()
        got2 = to_numpy(o2, PIPE_OUT)
        assert np.nonzero(got2 != got)[0].tolist() == [j6]
        assert (got2[j6]["stage"], got2[j6]["action"], got2[j6]["reason"]) == (6, 2, 149) and got[j4] == got2[j4]
    finally:
        for d in (dpB2, dpB, dpA):
            if d is not None:
                d.close()
