"""Shared by test_ref_diff.py (CPU oracle) and test_gpu_ref_diff.py (libgpuflow): the
comparison of an implementation's results with a recorded run of the reference programs
(tests/golden/ref_<program>_<case>.npz) through the mapping of oracle/REFDIFF.md."""
import os

import numpy as np

from oracle import refdiff as R, ref_cases as RC

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = list(RC.CASES)
_cache = {}


def fixture(program, case):
    key = (program, case)
    if key not in _cache:
        _cache[key] = R.load_fixture(os.path.join(GOLDEN, "ref_%s_%s.npz" % (program, case)))
    return _cache[key]


def scenario(case):
    """The case's scenario, regenerated once and shared: read-only (an OracleDP or Datapath built
    from it installs copies of the map contents and never writes the frames)."""
    key = ("sc", case)
    if key not in _cache:
        _cache[key] = RC.scenario(case)
    return _cache[key]


def dump_dict(kv):
    k, v = kv
    return {bytes(a): bytes(b) for a, b in zip(k, v)}


def check_unmodelled(fx):
    for b in fx["batches"]:
        assert int(b["obs"]["unmodelled"].sum()) == 0, "a packet reached an unmodelled helper"
        assert not np.any(b["obs"]["ret"] == R.LEFT), "a packet left through an unmodelled tail call"


def check_ingress_batch(b, pk, sc, out, frames=None):
    """out: ING_OUT records of an implementation for the batch recorded in b."""
    l4_off = R.plain_l4_off(pk)
    m = R.ingress_records(b, pk, sc.host_ifindex, l4_off)
    for f in ("action", "reason", "ifindex_lo"):
        assert np.array_equal(m[f], out[f]), "%s differs from the reference at %s" % (f, np.nonzero(m[f] != out[f])[0][:8])
    assert np.array_equal(m["proxied"], out["flags"] & 1), "proxy redirect flag differs from the reference"
    # the port is read from the frame the reference left, where the frame bytes alone say where it
    # is: the L4 header directly behind a plain IP header (with an IHL below 5 the port field
    # overlaps the addresses that the redirect stores afterwards) and inside the snap; every
    # proxy-map entry, whose key holds the port, is compared through the map dumps
    vis = (l4_off >= 0) & (l4_off + 4 <= pk.frames.shape[1])
    assert vis[m["proxied"] == 1].any() or not m["proxied"].any()
    assert np.array_equal(m["proxy_port"][vis], out["proxy_port"][vis]), "proxy_port differs from the reference"
    # the reason of a forwarded packet (ct_ret) shows only in a trace notification
    ev, own = R.events_160(b, pk.frames.shape[1])
    tr = ev[:, 0] == 4
    fwd = out["action"] != R.TC_ACT_SHOT
    assert np.all(fwd[own[tr]]), "a trace notification for a dropped packet"
    assert np.array_equal(ev[tr, 26], out["ct_ret"][own[tr]]), "ct_ret differs from the reference's trace reason"
    if frames is not None:
        bad = np.nonzero((b["frames"] != frames).any(axis=1))[0]
        assert len(bad) == 0, "frames differ from the reference at %s" % bad[:8]
    return m, ev, own


def check_lb_batch(b, pk, out, nd6, frames=None):
    m = R.lb_records(b, pk)
    assert np.array_equal(m["action"], out["action"]), "LB action differs at %s" % np.nonzero(m["action"] != out["action"])[0][:8]
    assert np.array_equal(m["reason"], out["reason"]), "LB reason differs"
    et = (pk.frames[:, 12].astype(np.uint32) << 8) | pk.frames[:, 13]
    x = out["action"] == R.TC_ACT_REDIRECT        # LB_REDIRECT is set: a translated frame is redirected
    x4, x6 = x & (et == 0x0800), x & (et == 0x86DD)
    assert np.array_equal(m["daddr4"][x4], out["new_daddr4"][x4]), "new_daddr4 differs from the frame the reference left"
    assert np.array_equal(m["daddr6"][x6], nd6[x6]), "new_daddr6 differs from the frame the reference left"
    obs = b["obs"]
    assert np.array_equal(obs["redirect_called"] == 1, x)
    if frames is not None:
        # DESIGN.md "Deviations kept on purpose": a frame the LB drops inside lb4_xlate / lb6_xlate
        # (DROP_CSUM_L4) keeps its original bytes, where the reference's skb already has the new
        # daddr (REFDIFF.md).  The reference's frame may differ from the input only there and only
        # in the daddr and the IPv4 header checksum; every other frame must equal the reference's.
        dev = lb_deviation_rows(b, pk, m)
        want = np.where(dev[:, None], pk.frames, b["frames"])
        bad = np.nonzero((want != frames).any(axis=1))[0]
        assert len(bad) == 0, "LB frames differ from the reference at %s" % bad[:8]
    return m


DROP_CSUM_L4 = 154


def lb_deviation_rows(b, pk, m=None):
    """The frames under the documented LB deviation: dropped with DROP_CSUM_L4.  Asserts that the
    reference changed no other dropped frame, and these only in the daddr (IPv4 30..33 plus the
    header checksum 24..25, IPv6 38..53)."""
    if m is None:
        m = R.lb_records(b, pk)
    shot = m["action"] == R.TC_ACT_SHOT
    dev = shot & (m["reason"] == DROP_CSUM_L4)
    diff = b["frames"] != pk.frames
    assert not diff[shot & ~dev].any(), "the reference changed a frame it dropped outside lb*_xlate"
    v6 = (pk.frames[:, 12] == 0x86) & (pk.frames[:, 13] == 0xDD)
    cols = np.arange(pk.frames.shape[1])
    may = np.where(v6[:, None], (cols >= 38) & (cols < 54), ((cols >= 30) & (cols < 34)) | (cols == 24) | (cols == 25))
    assert not (diff & ~may)[dev].any(), "the reference changed more than the daddr of a frame dropped in lb*_xlate"
    return dev


def lb_events_want(b, pk):
    """The reference's LB drop records with the payload of the deviation above: the header as
    the reference wrote it; the captured bytes of a DROP_CSUM_L4 frame from the input frame."""
    ev, own = R.events_160(b, pk.frames.shape[1])
    dev = lb_deviation_rows(b, pk)
    for r, i in zip(ev, own):
        if dev[i]:
            cap = min(int(r[12:16].view("<u4")[0]), pk.frames.shape[1])
            r[32:32 + cap] = pk.frames[i, :cap]
    return ev, own


def check_hand_expectations(fx, sc):
    """The hand-built case does what each packet is there for (oracle/ref_cases.hand): the
    reference's action, drop reason and, where a trace notification shows it, ct_ret per packet;
    the rev-NAT reply is rewritten; the CT entries at their lifetime boundary are found (not
    CT_NEW), counted and refreshed by the batch that probes them and untouched before."""
    rewritten = 0
    for bi, (b, pk, exp) in enumerate(zip(fx["batches"], sc.batches, sc.meta["expect"])):
        assert len(exp) == pk.n
        m = R.ingress_records(b, pk, sc.host_ifindex, R.plain_l4_off(pk))
        ev, own = R.events_160(b, pk.frames.shape[1])
        for i, (action, reason, ct, what) in enumerate(exp):
            assert (int(m["action"][i]), int(m["reason"][i])) == (action, reason), "batch %d packet %d: %s" % (bi, i, what)
            tr = ev[(own == i) & (ev[:, 0] == 4)]
            if ct is None:
                assert len(tr) == 0, "batch %d packet %d: %s" % (bi, i, what)
            else:
                assert len(tr) == 1 and int(tr[0, 26]) == ct, "batch %d packet %d: %s" % (bi, i, what)
            if "rev-NAT index: source rewritten" in what:
                assert bytes(b["frames"][i, 26:30]) == bytes([10, 96, 0, 1]) != bytes(pk.frames[i, 26:30])
                rewritten += 1
    assert rewritten == 1
    ct0 = dict(zip(map(bytes, sc.maps["ct4"].keys), map(bytes, sc.maps["ct4"].vals)))
    nows = RC.nows(sc)
    for key, probe in sc.meta["boundary"]:
        assert int.from_bytes(ct0[key][32:36], "little") in (nows[probe], nows[probe] - 1)
        for bi, b in enumerate(fx["batches"]):
            v = dump_dict(b["maps"]["ct4"])[key]
            if bi < probe:
                assert v == ct0[key], "boundary entry touched before its probe"
            else:
                assert int.from_bytes(v[0:8], "little") == 1, "boundary entry: rx packets did not move"
                assert int.from_bytes(v[32:36], "little") == nows[probe] + 43200, "boundary entry: lifetime not refreshed"
    probes = {p for _, p in sc.meta["boundary"]}
    for p in probes:
        assert sc.meta["expect"][p][0][2] == 2          # the probing packet is expected as CT_REPLY
