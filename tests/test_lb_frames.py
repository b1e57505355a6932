"""bpf_lb over raw frames (gf_lb_classify_frames), CPU side: tests/lb_frames_model.py against the
hand-derived KATs and against the oracle's pipeline wherever the oracle runs bpf_lb to its end."""
import numpy as np
import pytest

from cilium_amd import synth
from oracle.scenario import OracleDP
from tests import lb_frames_model as LM

STAGE_LB = 2                                            # GF_STAGE_LB
# what the program can answer send_drop_notify_error with: revalidate_data, l4_load_port's
# -EFAULT, lb*_lookup_slave, csum_l4_replace.  DROP_WRITE_ERROR (l4_modify_port's store) needs a
# frame whose checksum field lies inside it and whose port does not: no such TCP / UDP frame.
DROP_REASONS = (LM.EFAULT, LM.DROP_INVALID, LM.DROP_CSUM_L4, LM.DROP_NO_SERVICE)

DOC = LM.load_kats()


@pytest.fixture(scope="module")
def anchor():
    """(scenario, [(packets, oracle records, oracle nd6, oracle frames, model records, nd6, frames)])"""
    sc = synth.lb_frames_fuzz(seed=3, n_packets=3000, n_batches=2)
    assert sc.xdp is None and sc.lb["flags"] & synth.LB_REDIRECT
    ref, m = OracleDP(sc), LM.LbFramesModel(sc)
    return sc, [(pk,) + tuple(ref.pipeline(pk, sc.now + bi)) + m.batch(pk) for bi, pk in enumerate(sc.batches)]


def kat_ids():
    return [k["name"] for k in DOC["kats"]]


def test_kat_file_covers_the_listed_cases():
    names = set(kat_ids())
    assert len(names) == len(DOC["kats"])
    for want in ("v4_tcp_l4_redirect_dstmac", "v4_tcp_l4_redirect_nomac", "v4_udp_l4_slave2", "v4_udp_csum0_left_alone",
                 "v4_udp_update_yields_0_becomes_ffff", "v4_tcp_l3_fallback_port0_quirk", "v4_options_tcp",
                 "v6_tcp_revnat_or_no_redirect", "v6_udp_behind_hopopts", "v4_icmp_no_l3_service", "v4_gre_unknown_l4_ok",
                 "arp", "v4_cut_in_ip_header", "v4_tcp_csum_past_end", "v4_udp_missing_slave", "no_ipv4_flag", "no_ipv6_flag"):
        assert want in names


@pytest.mark.parametrize("kat", DOC["kats"], ids=kat_ids())
def test_model_reproduces_kat(kat):
    sc = LM.kat_scenario(DOC, kat["flags"], kat["dstmac"])
    pk, recs, nd6, out = LM.kat_packets(DOC, [kat])
    r, n6, f = LM.LbFramesModel(sc).batch(pk)
    assert r[0] == recs[0], (r[0], recs[0])
    assert np.array_equal(n6, nd6)
    assert np.array_equal(f, out), np.nonzero(f[0] != out[0])[0]


def test_kat_expectations_are_consistent():
    """The hand-derived outputs verify as checksums (except the documented quirk), an untouched
    frame's output is its input, and a translated record names the address the output carries."""
    for k in DOC["kats"]:
        pk, recs, nd6, out = LM.kat_packets(DOC, [k])
        f, o, n = pk.frames[0], out[0], int(pk.lens[0])
        translated = bool(recs["slave"][0])
        if not translated:
            assert np.array_equal(f, o), k["name"]
            continue
        v4 = bytes(o[12:14]) == b"\x08\x00"
        if v4:
            assert LM.ip4_header_ok(o), k["name"]
            assert int.from_bytes(bytes(o[30:34]), "little") == recs["new_daddr4"][0]
        else:
            assert np.array_equal(o[38:54], nd6[0])
        proto = int(o[23]) if v4 else (int(o[20]) or int(o[54]))
        l4 = 14 + (o[14] & 0xf) * 4 if v4 else 54
        udp0 = proto == 17 and not o[l4 + 6] and not o[l4 + 7]
        if proto in (6, 17) and not udp0 and (v4 or o[20]) and "quirk" not in k["name"]:
            assert LM.l4_ok(o, n), k["name"]
        if "quirk" in k["name"]:
            assert not LM.l4_ok(o, n)


def test_model_anchored_on_oracle(anchor):
    """Every frame the oracle's pipeline ends at GF_STAGE_LB (SHOT, or REDIRECT under LB_REDIRECT)
    has the model's record, and a redirected one the model's bytes; the anchored share is large."""
    sc, runs = anchor
    n = redirect = 0
    reasons = set()
    for pk, ro, rn6, rs, mr, mn6, mf in runs:
        lb = ro["stage"] == STAGE_LB
        # the two agree on which frames the program ends
        assert np.array_equal(lb, (mr["action"] == LM.TC_ACT_SHOT) | (mr["action"] == LM.TC_ACT_REDIRECT))
        for a, b in (("action", "action"), ("reason", "reason")):
            assert np.array_equal(mr[a][lb], ro[b][lb]), a
        rd = lb & (ro["action"] == LM.TC_ACT_REDIRECT)
        for a, b in (("slave", "slave"), ("rev_nat", "rev_nat"), ("new_dport", "dport"), ("new_daddr4", "daddr4")):
            assert np.array_equal(mr[a][rd], ro[b][rd]), a
        assert np.array_equal(mn6[rd], rn6[rd])
        assert np.array_equal(mf[rd], rs[rd])
        sh = lb & (ro["action"] == LM.TC_ACT_SHOT)
        assert not mr["slave"][sh].any() and not mn6[sh].any()
        assert np.array_equal(mf[sh], pk.frames[sh])     # a dropped frame keeps its bytes
        n += pk.n
        redirect += int(rd.sum())
        reasons |= set(int(x) for x in ro["reason"][sh])
    assert redirect * 4 >= n, (redirect, n)
    assert reasons == set(DROP_REASONS), reasons


def test_untranslated_frames_keep_every_byte(anchor):
    sc, runs = anchor
    for pk, ro, rn6, rs, mr, mn6, mf in runs:
        same = mr["slave"] == 0
        assert same.any() and np.array_equal(mf[same], pk.frames[same])
        # and a translated one changes nothing outside the fields the reference writes
        for i in np.nonzero(~same)[0][:200]:
            v4 = bytes(pk.frames[i, 12:14]) == b"\x08\x00"
            ch = set(np.nonzero(mf[i] != pk.frames[i])[0].tolist())
            l4 = 14 + (int(pk.frames[i, 14]) & 0xf) * 4 if v4 else None
            if v4:
                co = LM.M.csum_offset(int(pk.frames[i, 23]))
                allowed = {24, 25, 30, 31, 32, 33, l4 + 2, l4 + 3} | ({l4 + co, l4 + co + 1} if co else set())
                assert ch <= allowed, (i, sorted(ch - allowed))
            else:
                assert not [x for x in ch if x < 38], (i, sorted(ch))


def test_valid_checksums_stay_valid():
    """RFC 1624: frames with correct checksums still verify after the rewrite, except where the
    L3-fallback translation updates the L4 checksum from port 0 (DESIGN.md's quirk)."""
    sc = synth.lb_frames_fuzz(seed=5, n_packets=1500, n_batches=1)
    pk = sc.batches[0]
    S = pk.frames.shape[1]
    et = (pk.frames[:, 12].astype(int) << 8) | pk.frames[:, 13]
    v4 = et == 0x0800
    whole = np.array([(v4[i] and pk.frames[i, 14] & 0xf >= 5 and 34 <= pk.lens[i] <= S and pk.frames[i, 23] in (6, 17)
                       and pk.lens[i] >= 14 + (pk.frames[i, 14] & 0xf) * 4 + (20 if pk.frames[i, 23] == 6 else 8))
                      or (et[i] == 0x86DD and pk.frames[i, 20] in (6, 17) and 54 + 20 <= pk.lens[i] <= S)
                      for i in range(pk.n)])
    idx = np.nonzero(whole)[0]
    for i in idx:
        LM.set_checksums(pk.frames[i], int(pk.lens[i]))
        assert LM.l4_ok(pk.frames[i], int(pk.lens[i]))
    m = LM.LbFramesModel(sc)
    recs, nd6, fr = m.batch(pk)
    checked = quirk = 0
    for i in idx:
        if not recs["slave"][i]:
            continue
        n = int(pk.lens[i])
        if v4[i]:
            assert LM.ip4_header_ok(fr[i]), i
            key = bytes(pk.frames[i, 30:34]) + bytes(pk.frames[i, 14 + (pk.frames[i, 14] & 0xf) * 4 + 2:][:2]) + b"\0\0"
            tab = m.lb4
        else:
            key = bytes(pk.frames[i, 38:54]) + bytes(pk.frames[i, 56:58]) + b"\0\0"
            tab = m.lb6
        l4_hit = key in tab and int.from_bytes(tab[key][len(tab[key]) - 6:][:2], "little")
        if recs["new_dport"][i] and not l4_hit:
            quirk += 1                                  # port rewritten after the L3 fallback: from port 0
            assert not LM.l4_ok(fr[i], n), i
        else:
            assert LM.l4_ok(fr[i], n), i
            checked += 1
    assert checked >= 100 and quirk >= 1, (checked, quirk)


def test_comparisons_bite(anchor):
    """A flipped frame byte or record field is seen by the comparisons the tests use."""
    sc, runs = anchor
    pk, ro, rn6, rs, mr, mn6, mf = runs[0]
    rd = np.nonzero((ro["stage"] == STAGE_LB) & (ro["action"] == LM.TC_ACT_REDIRECT))[0]
    f2 = mf.copy()
    f2[rd[0], 31] ^= 1
    assert not np.array_equal(f2[rd], rs[rd])
    for name in LM.LB_OUT.names:
        r2 = mr.copy()
        r2[name][rd[-1]] ^= 1
        assert not np.array_equal(r2, mr)
        assert not np.array_equal(r2.view(np.uint8), mr.view(np.uint8))
    ev = LM.drop_events(pk, mr, mf)
    assert len(ev) == int((mr["action"] == LM.TC_ACT_SHOT).sum()) > 0
    e2 = ev.copy()
    e2[0, 33] ^= 1
    assert not np.array_equal(e2, ev)


def test_drop_records_equal_the_oracles(anchor):
    """The model's send_drop_notify_error records are the oracle pipeline's for the frames dropped
    at GF_STAGE_LB (the oracle's other drops come from later programs)."""
    sc, runs = anchor
    ref = OracleDP(sc)
    pk = sc.batches[0]
    ro, rn6, rs, ev = ref.pipeline(pk, sc.now, events=True)
    shot = np.nonzero(ro["action"] == LM.TC_ACT_SHOT)[0]
    assert len(ev) == len(shot)
    at_lb = ro["stage"][shot] == STAGE_LB
    mr, mn6, mf = runs[0][4:]
    mine = LM.drop_events(pk, mr, mf)
    assert at_lb.sum() == len(mine) > 0
    assert np.array_equal(ev[at_lb], mine)


def test_dstmac_and_redirect_variants():
    """LB_DSTMAC touches bytes 0-5 of exactly the redirected frames; without LB_REDIRECT the same
    frames are translated and answered TC_ACT_OK."""
    mac = bytes.fromhex("aabbccddeeff")
    sc = synth.lb_frames_fuzz(seed=3, n_packets=1200, n_batches=1, dstmac=mac)
    assert sc.lb["dstmac"] == mac
    pk = sc.batches[0]
    r1, n1, f1 = LM.LbFramesModel(sc).batch(pk)
    r0, n0, f0 = LM.LbFramesModel(sc, dstmac=None).batch(pk)
    assert np.array_equal(r1, r0) and np.array_equal(n1, n0)
    rd = r1["action"] == LM.TC_ACT_REDIRECT
    assert rd.any() and (f1[rd, :6] == np.frombuffer(mac, np.uint8)).all()
    assert np.array_equal(f1[:, 6:], f0[:, 6:]) and np.array_equal(f1[~rd], f0[~rd])
    assert np.array_equal(f0[:, :6], pk.frames[:, :6])
    r2, n2, f2 = LM.LbFramesModel(sc, flags=sc.lb["flags"] & ~synth.LB_REDIRECT, dstmac=None).batch(pk)
    assert np.array_equal(f2, f0) and np.array_equal(n2, n0)
    assert not (r2["action"] == LM.TC_ACT_REDIRECT).any()
    assert np.array_equal(r2["action"][rd], np.zeros(rd.sum(), np.uint8))
    for name in ("reason", "slave", "new_dport", "rev_nat", "new_daddr4"):
        assert np.array_equal(r2[name], r0[name])


def test_scenario_changes_nothing_existing():
    """The dstmac key and lb_frames_fuzz leave the scenarios the goldens were made from alone."""
    a, b = synth.pipeline_fuzz(seed=3, n_packets=500, n_batches=1), synth.pipeline_fuzz(seed=3, n_packets=500, n_batches=1)
    synth.lb_frames_fuzz(seed=3, n_packets=500, n_batches=1)
    assert "dstmac" not in a.lb and a.lb == b.lb
    assert np.array_equal(a.batches[0].frames, b.batches[0].frames)
