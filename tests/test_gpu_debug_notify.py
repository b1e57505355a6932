"""Debug notifications on the GPU (GF_LXC_F_DEBUG, k_ing_groups_dbg + the event pass):
the ring, decoded with cilium_amd.monitor, against the per-packet lists of
tests/dbg_model.py concatenated in batch order (debug, trace and drop records
together); verdicts and CT maps against the C oracle, which also anchors the model."""
import ctypes as C
import errno

import numpy as np
import pytest

from cilium_amd import monitor as MON
from cilium_amd import synth
from oracle.scenario import OracleDP
from tests import dbg_model as M
from tests.test_debug_notify import LXC_DEBUG, NOW, kats, packets, run_anchored, scenario

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(0)


class Ring:
    def __init__(self, cap):
        from cilium_amd._lib import lib, gf_event_ring
        self.lib, self.cap = lib, cap
        self.recs = torch.zeros((max(cap, 1), 160), dtype=torch.uint8, device="cuda")
        self.cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
        self.ring = gf_event_ring(self.recs.data_ptr(), cap, self.cnt.data_ptr())

    def __enter__(self):
        assert self.lib.gf_set_event_ring(C.byref(self.ring)) == 0
        return self

    def __exit__(self, *a):
        self.lib.gf_set_event_ring(None)

    def raw(self):
        torch.cuda.synchronize()
        n = int(self.cnt.item())
        return n, self.recs[:min(n, self.cap)].cpu().numpy()


def _check_ring(raw, want, what=""):
    got = MON.decode_ring(raw)
    assert len(got) == len(want), (what, len(got), len(want))
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, (what, k, g, w)
    for k, g in enumerate(got):                                   # zero fill past what the reference writes
        end = 20 if g["type"] == 2 else (24 if g["type"] == 3 else 32) + g["len_cap"]
        assert not raw[k, end:].any(), (what, k)


def _gpu_run(sc, batches, nows, batches_api=False):
    from cilium_amd.datapath import Datapath, DeviceBatch, ING_OUT, to_numpy
    dp = Datapath(sc, pin_prefix=None)
    dbs = [DeviceBatch(pk) for pk in batches]
    if batches_api:
        outs = dp.ingress_batches(dbs, nows)
    else:
        outs = [dp.ingress(db, now) for db, now in zip(dbs, nows)]
    torch.cuda.synchronize()
    return dp, [to_numpy(o, ING_OUT) for o in outs]


def _full(sc, batches, nows, what, batches_api=False, cap=4096):
    """GPU vs model (ring) and vs oracle (records, CT maps, policy counters, proxy maps)."""
    model, recs, evs = run_anchored(sc, batches, nows, what)
    want = [e for ev in evs for per_packet in ev for e in per_packet]
    with Ring(cap) as ring:
        dp, outs = _gpu_run(sc, batches, nows, batches_api)
        n, raw = ring.raw()
    for got, ref in zip(outs, recs):
        assert np.array_equal(got, ref), what
    assert n == len(want), (what, n, len(want))
    _check_ring(raw, want[:cap], what)
    ref = OracleDP(sc)
    for pk, now in zip(batches, nows):
        ref.ingress(pk, now)
    for name in list(model.ct) + [e["policy"] for e in sc.lxc] + ["cilium_proxy4", "cilium_proxy6"]:
        assert dp.dump_map(name) == ref.dump(name), (what, name)
    return raw, want


def _kat_batch():
    """The KAT traffic as one batch on 4 endpoints (0 and 2 with the flag), IPv4 and IPv6
    together: every case's packets towards each endpoint in turn, each case from a source
    address of its own so that the cases do not share conntrack entries."""
    specs, prefill = [], []
    for ci, c in enumerate(kats()):
        if c.get("ct"):
            continue                                               # (its own CT map type: CPU only)
        if c.get("prefill"):                                       # prefilled entries are endpoint 0's, from the KAT source
            prefill += [q for q in c["prefill"] if q not in prefill]
            specs += [dict(p, ep=0, src=0) for p in c["packets"]]
        else:
            for ep in (ci % 4, (ci + 1) % 4):                      # once to an endpoint with the flag, once without
                specs += [dict(p, ep=ep, src=ci + 1) for p in c["packets"]]
    return specs, prefill


def test_kat_traffic_one_batch_four_endpoints():
    """Fails without the feature: the ring then holds no type-2/3 record."""
    _gpu()
    specs, prefill = _kat_batch()
    assert 15 <= len(specs) <= 45
    sc = scenario(n_ep=4, debug=(0, 2), prefill=prefill)
    raw, want = _full(sc, [packets(specs)], [NOW], "kats")
    types = raw[:, 0]
    assert (types == 2).sum() > 20 and (types == 3).sum() >= 1 and (types == 4).sum() > 5 and (types == 1).sum() >= 2
    dbg_src = {int(s) for s in raw[:, 2:4].copy().view("<u2")[:, 0][(types == 2) | (types == 3)]}
    assert dbg_src <= {100, 102}                                   # endpoints 1 and 3 contribute no type-2/3 record


def test_one_flow_group_six_packets():
    """Six packets of one connection in one bucket, on an entry the other side has already
    closed (tx_closing, lifetime 7777): FIN (both sides closing: now + CT_CLOSE_TIMEOUT), a
    SYN that re-opens it (now + CT_DEFAULT_LIFETIME), ACK, data, FIN, SYN.  Every DBG_CT_MATCH
    lifetime is the value the previous packet of the group left, so the log is written per
    packet in bucket order, not per bucket.  (Within one call `now` is fixed and an open TCP
    entry that has seen a non-SYN only ever gets now + CT_DEFAULT_LIFETIME, so the last four
    values cannot differ; the ring is also compared record by record with the model.)"""
    _gpu()
    t = dict(id=1000, proto="tcp", dport=80)
    specs = [dict(t, tcp_flags=f) for f in (17, 2, 16, 24, 17, 2)]
    sc = scenario(prefill=[dict(sport=40000, dport=80, proto="tcp", lifetime=7777, forward=True, ct_flags=2 | 16)])
    raw, want = _full(sc, [packets(specs)], [NOW], "group")
    match = [e["arg1"] for e in MON.decode_ring(raw) if e.get("name") == "DBG_CT_MATCH"]
    assert match == [7777, NOW + 10, NOW + 43200, NOW + 43200, NOW + 43200, NOW + 43200], match


def test_ct_create_failed_on_full_hash_map():
    """DBG_CT_CREATED4 is sent before the map update: also when the packet ends in
    DROP_CT_CREATE_FAILED (a HASH CT map of max_entries 1 that holds an unrelated entry)."""
    _gpu()
    sc = scenario(ct={"type": "hash", "max_entries": 1}, prefill=[dict(sport=1, dport=2, proto="udp", lifetime=9000)])
    raw, want = _full(sc, [packets([dict(id=1000, proto="tcp", dport=80, tcp_flags=2)])], [NOW], "ct full")
    names = [e.get("name", "DROP") for e in MON.decode_ring(raw)]
    assert names[-2:] == ["DBG_CT_CREATED4", "DROP"] and raw[-1, 1] == 155


def test_proxymap_create_failed():
    """A redirect that ends in DROP_PROXYMAP_CREATE_FAILED has sent the capture and
    DBG_REV_PROXY_UPDATE but not DBG_TO_HOST (cilium_proxy4 with max_entries 1)."""
    _gpu()
    specs = [dict(id=1000, proto="tcp", dport=8080, tcp_flags=2, src=k) for k in range(3)]
    raw, want = _full(scenario(px_max=1), [packets(specs)], [NOW], "px full")
    names = [e.get("name", "DROP") for e in MON.decode_ring(raw)]
    assert names.count("DBG_TO_HOST") == 1 and names.count("DBG_REV_PROXY_UPDATE") == 3
    assert names[-2:] == ["DBG_REV_PROXY_UPDATE", "DROP"] and raw[-1, 1] == 161


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_batch_sizes(n):
    """Every packet a debug packet of one of three flows: the event pass's block and wave
    boundaries with several records per packet."""
    _gpu()
    flows = [dict(id=1000, proto="tcp", dport=80, tcp_flags=16), dict(id=1000, proto="udp", dport=53),
             dict(id=1000, proto="tcp", dport=8080, tcp_flags=16, family=6)]
    specs = [dict(flows[k % 3], src=1 + (k % 3)) for k in range(n)]
    _full(scenario(), [packets(specs)], [NOW], f"n{n}")


def test_ring_smaller_than_the_records():
    _gpu()
    specs = [dict(id=1000, proto="tcp", dport=80, tcp_flags=2, src=k + 1) for k in range(20)]
    raw, want = _full(scenario(), [packets(specs)], [NOW], "small ring", cap=37)
    assert len(want) == 20 * 8 and len(raw) == 37                  # the prefix present, *count the full number


def test_no_ring_and_ring_without_a_debug_program():
    _gpu()
    specs, prefill = _kat_batch()
    pk = packets(specs)
    # no ring: records, CT maps and policy counters equal the oracle's
    sc = scenario(n_ep=4, debug=(0, 2), prefill=prefill)
    dp, outs = _gpu_run(sc, [pk], [NOW])
    ref = OracleDP(sc)
    assert np.array_equal(outs[0], ref.ingress(pk, NOW))
    for name in ["ct4", "ct6"] + [e["policy"] for e in sc.lxc]:
        assert dp.dump_map(name) == ref.dump(name), name
    # a ring, no program with the flag: today's records only (the model without the flag restates them)
    plain = scenario(n_ep=4, debug=(), prefill=prefill)
    raw, want = _full(plain, [pk], [NOW], "no debug program")
    assert len(raw) > 10 and not ((raw[:, 0] == 2) | (raw[:, 0] == 3)).any()
    # ... and byte for byte the ring of an array that held programs with the flag and was
    # then updated to programs without it (gf_policy_array_update resets the array's bit)
    from cilium_amd._lib import lib
    from cilium_amd.datapath import Datapath, DeviceBatch, ING_OUT, to_numpy
    was = Datapath(scenario(n_ep=4, debug=(0, 1, 2, 3), prefill=prefill), pin_prefix=None)
    now_ = Datapath(plain, pin_prefix=None)                        # its programs (and their maps) replace the flagged ones
    for e, prog in zip(plain.lxc, now_.lxc_progs):
        assert lib.gf_policy_array_update(was.policy_array, e["lxc_id"], prog) == 0
    with Ring(4096) as ring:
        out = was.ingress(DeviceBatch(pk), NOW)
        n, raw2 = ring.raw()
    assert np.array_equal(to_numpy(out, ING_OUT), OracleDP(plain).ingress(pk, NOW))
    assert n == len(raw) and raw2.tobytes() == raw.tobytes()


def test_conntrack_local_three_endpoints():
    """Per-endpoint CT maps (the PCT instantiation), two of three endpoints with the flag."""
    _gpu()
    specs = []
    for k in range(24):
        specs.append(dict(id=1000, proto="tcp", dport=(80, 8080)[k % 2], tcp_flags=(2, 16)[(k // 6) % 2], ep=k % 3,
                          src=1 + k % 2, family=(4, 6)[(k // 3) % 2]))
    _full(scenario(n_ep=3, debug=(0, 1), local=True), [packets(specs)], [NOW], "local")


def test_batches_api_second_batch_sees_first_batchs_lifetime():
    _gpu()
    b1 = packets([dict(id=1000, proto="tcp", dport=80, tcp_flags=2)])
    b2 = packets([dict(id=1000, proto="tcp", dport=80, tcp_flags=16)])
    raw, want = _full(scenario(), [b1, b2], [NOW, NOW + 7], "batches", batches_api=True)
    match = [e["arg1"] for e in MON.decode_ring(raw) if e.get("name") == "DBG_CT_MATCH"]
    assert match == [NOW + 300]


def test_debug_with_no_conntrack_is_refused():
    _gpu()
    from cilium_amd._lib import lib, gf_lxc_cfg
    cfg = gf_lxc_cfg()
    cfg.lxc_id, cfg.seclabel = 7, 300
    cfg.flags = synth.LXC_POLICY_INGRESS | synth.LXC_LXC_IPV4 | synth.LXC_NO_CONNTRACK | LXC_DEBUG
    assert lib.gf_lxc_prog_load(C.byref(cfg)) == -errno.EOPNOTSUPP


def test_pipeline_ignores_the_flag():
    """gf_pipeline_classify over a few frames to a program with the flag: the same records
    and the same ring bytes as without it."""
    _gpu()
    from cilium_amd.datapath import Datapath, DeviceBatch, PIPE_OUT, to_numpy
    res = []
    for flagged in (False, True):
        sc = synth.pipeline_fuzz(seed=3, n_packets=300, n_batches=1)
        for e in sc.lxc:
            e["flags"] |= synth.LXC_TRACE_NOTIFY | (LXC_DEBUG if flagged and not e["flags"] & synth.LXC_NO_CONNTRACK else 0)
        with Ring(4096) as ring:
            dp = Datapath(sc, pin_prefix=None)
            out, nd6, snap = dp.pipeline(DeviceBatch(sc.batches[0], parse=False), sc.now)
            n, raw = ring.raw()
        res.append((to_numpy(out, PIPE_OUT).tobytes(), n, raw.tobytes()))
    assert res[0] == res[1] and res[0][1] > 0
