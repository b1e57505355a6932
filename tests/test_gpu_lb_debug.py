"""The DebugLB option on the GPU (GF_LXC_F_LB_DEBUG with GF_LXC_F_DEBUG: k_ing_groups_dbg's
reverse-NAT log bits and the event pass): the ring, decoded with cilium_amd.monitor, against
the per-packet lists of tests/lbdbg_model.py concatenated in batch order; verdicts, CT maps,
policy counters and proxy maps against the C oracle, which also anchors the model.  CT
entries with a rev_nat_index are preloaded through the map API (the scenario's map
contents)."""
import numpy as np
import pytest

from cilium_amd import monitor as MON
from cilium_amd import synth
from oracle.scenario import OracleDP
from tests.test_debug_notify import LXC_DEBUG, NOW
from tests.test_gpu_debug_notify import Ring, _check_ring, _gpu, _gpu_run
from tests.test_lb_debug import (BOTH, LXC_LB_DEBUG, all_replies, alternating_group, kat_batch, lb_names, local_three,
                                 packets, run_anchored, scenario, v6_mix, without_flag)

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


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


def _lb(raw):
    return [e for e in MON.decode_ring(raw) if e.get("name", "").startswith("DBG_LB")]


def test_kat_traffic_one_batch_four_endpoints():
    """Endpoints with DEBUG | LB_DEBUG, DEBUG only, LB_DEBUG only, neither.  Fails without the
    feature: the ring then holds no DBG_LB* record."""
    _gpu()
    flags, specs, prefill = kat_batch()
    assert 30 <= len(specs) <= 60
    raw, want = _full(scenario(flags, prefill), [packets(specs)], [NOW], "kats")
    lb = _lb(raw)
    assert len(lb) == 12 and {e["source"] for e in lb} == {100}    # only the endpoint with both flags
    assert {e["name"] for e in lb} == {"DBG_LB4_REVERSE_NAT_LOOKUP", "DBG_LB4_REVERSE_NAT", "DBG_LB6_REVERSE_NAT_LOOKUP",
                                       "DBG_LB6_REVERSE_NAT"}
    dbg_src = {e["source"] for e in MON.decode_ring(raw) if e["type"] in (2, 3)}
    assert dbg_src == {100, 101}                                   # LB_DEBUG alone sends nothing


def test_flag_cleared_gives_the_parent_ring():
    """The KAT batch with LB_DEBUG cleared on every program: the Debug ring as before the option
    existed.  The expectation is lbdbg_model with the flag clear, in which every record comes from
    dbg_model's own call sites; dbg_model alone cannot run this batch (it asserts the reverse NAT
    absent, whose verdicts the subclass adds).  tests/test_lb_debug.py shows the two models equal
    where dbg_model applies."""
    _gpu()
    flags, specs, prefill = kat_batch()
    sc = without_flag(scenario(flags, prefill))
    assert not any(e["flags"] & LXC_LB_DEBUG for e in sc.lxc) and any(e["flags"] & LXC_DEBUG for e in sc.lxc)
    raw, want = _full(sc, [packets(specs)], [NOW], "flag cleared")
    assert not _lb(raw) and (raw[:, 0] == 2).sum() > 40


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_batch_sizes(n):
    """Every packet a reverse-NAT reply (hit with port, hit without, miss in turn): wave and block
    boundaries of the log column and of the event scan."""
    _gpu()
    specs, prefill = all_replies(n)
    raw, want = _full(scenario(prefill=prefill), [packets(specs)], [NOW], f"n{n}")
    assert len(_lb(raw)) == sum(2 if k % 3 < 2 else 1 for k in range(n))


def test_one_flow_group_alternating_directions():
    """Six packets of one flow group, reply and forward direction in turn (the bucket key is the
    unordered address pair): one lane runs all six, and only the replies log the lookup."""
    _gpu()
    specs, prefill = alternating_group()
    raw, want = _full(scenario(prefill=prefill), [packets(specs)], [NOW], "group")
    assert [e["name"] for e in _lb(raw)] == ["DBG_LB4_REVERSE_NAT_LOOKUP", "DBG_LB4_REVERSE_NAT"] * 3
    verdicts = [(e["arg1"], e["arg2"]) for e in MON.decode_ring(raw) if e.get("name") == "DBG_CT_VERDICT"]
    assert verdicts == [(2, 0x0700), (1, 0x0800)] * 3


def test_ipv6_hit_miss_established_and_failed_rewrite():
    _gpu()
    specs, prefill = v6_mix()
    raw, want = _full(scenario(prefill=prefill), [packets(specs)], [NOW], "v6")
    names = [e.get("name", "DROP") for e in MON.decode_ring(raw)]
    assert names.count("DBG_LB6_REVERSE_NAT_LOOKUP") == 5 and names.count("DBG_LB6_REVERSE_NAT") == 4
    k = names.index("DROP")                                       # the extension-header frame: messages, then the drop
    assert names[k - 2:k] == ["DBG_LB6_REVERSE_NAT_LOOKUP", "DBG_LB6_REVERSE_NAT"] and raw[k, 1] == 154


def test_conntrack_local_three_endpoints():
    """Per-endpoint CT maps (the PCT instantiation); the third endpoint has DEBUG only."""
    _gpu()
    flags, specs, prefill = local_three()
    raw, want = _full(scenario(flags, prefill, local=True), [packets(specs)], [NOW], "local")
    assert {e["source"] for e in _lb(raw)} == {100, 101}


def test_ring_smaller_than_the_records():
    """As tests/test_gpu_debug_notify.py pins it for Debug: the prefix present, *count the full
    number; here the cut falls among packets whose lists hold LB records."""
    _gpu()
    specs, prefill = all_replies(20)
    raw, want = _full(scenario(prefill=prefill), [packets(specs)], [NOW], "small ring", cap=37)
    assert len(raw) == 37 and len(want) > 120
    assert lb_names(want[:37]) and lb_names(want[37:])


def test_batches_api_second_batch_on_first_batchs_entries():
    """The ingress entry point alone cannot create an IPv4 entry with an index (ct_create4 on ingress
    stores rev_nat_index 0), so the entries are preloaded; the first batch's replies refresh them, and the
    second batch's DBG_CT_MATCH reports the lifetime the first batch left, next to the same LB records."""
    _gpu()
    specs, prefill = all_replies(3)
    raw, want = _full(scenario(prefill=prefill), [packets(specs), packets(specs)], [NOW, NOW + 7], "batches",
                      batches_api=True)
    match = [e["arg1"] for e in MON.decode_ring(raw) if e.get("name") == "DBG_CT_MATCH"]
    assert match == [9000] * 3 + [NOW + 43200] * 3
    assert len(_lb(raw)) == 2 * 5


def test_pipeline_ignores_the_flag():
    """gf_pipeline_classify over a few frames to DEBUG | LB_DEBUG programs: the same records and
    the same ring bytes as with both flags clear."""
    _gpu()
    from cilium_amd.datapath import Datapath, DeviceBatch, PIPE_OUT, to_numpy
    res = []
    for flagged in (False, True):
        sc = synth.pipeline_fuzz(seed=3, n_packets=300, n_batches=1)
        for e in sc.lxc:
            e["flags"] |= synth.LXC_TRACE_NOTIFY
            if flagged:                                            # (DEBUG | NO_CONNTRACK is refused at load)
                e["flags"] |= LXC_LB_DEBUG if e["flags"] & synth.LXC_NO_CONNTRACK else BOTH
        with Ring(4096) as ring:
            dp = Datapath(sc, pin_prefix=None)
            out, nd6, snap = dp.pipeline(DeviceBatch(sc.batches[0], parse=False), sc.now)
            n, raw = ring.raw()
        res.append((to_numpy(out, PIPE_OUT).tobytes(), n, raw.tobytes()))
    assert res[0] == res[1] and res[0][1] > 0
