"""The CPU oracle against the reference programs themselves, executed as host code.

oracle/refdiff.py compiles bpf_lxc.c (handle_policy) and bpf_lb.c (from-netdev) of the
reference against a helper shim of our own and runs them packet by packet; what each run left
behind is recorded in tests/golden/ref_<program>_<case>.npz (tests/golden/make_ref_golden.py).
oracle/REFDIFF.md maps those observables onto the records.  Cases (oracle/ref_cases.py):

  fuzz1, fuzz2   synth.fuzz, n_ep=4, 2 batches of 2000 packets, CT state carried, now + 1 per batch
  hand           <= 200 packets: TCP SYN / SYN-ACK / ACK / FIN and the tuple reused, an RST, an ICMP
                 error related to a live entry (forwarded as CT_RELATED) and one that is not, a reply
                 rewritten by rev-NAT, CT entries probed at now == lifetime and at lifetime + 1, proxy
                 redirects (L4 list and the policy entry's own port), a CIDR-only allow (IPv4; IPv6 as
                 written, where the lookup sees the endpoint's own address), a fragment header,
                 nexthdr 59, three- (walked), four- and five-deep (both given up) extension chains,
                 AUTH headers, services with one and with three backends, a UDP checksum of 0 through
                 the LB rewrite.  test_hand_case_reaches_what_it_is_built_for asserts, per packet,
                 the outcome that oracle/ref_cases.py derives from the reference's text.

(a) with oracle/_ref/ present the runners run again and must reproduce the fixtures;
(b) the regenerated input hashes to the fixture's value;
(c) OracleDP (and, for bpf_lb's frames and events, tests/lb_frames_model.py) equals the fixture;
(d) the shim's checksum helpers equal a big-integer fold.
"""
import random

import numpy as np
import pytest

from oracle import refdiff as R, ref_cases as RC
from oracle import oracle as O
from oracle.scenario import OracleDP
from tests import ref_diff_common as D
from tests import lb_frames_model as LM

PROGRAMS = list(RC.PROGRAMS)


@pytest.mark.parametrize("case", D.CASES)
@pytest.mark.parametrize("program", PROGRAMS)
def test_a_runner_reproduces_fixture(program, case):
    if not R.has_runner():
        pytest.skip("oracle/_ref/ absent: no reference checkout on this machine")
    sc = RC.scenario(case)
    got = R.fixture_arrays(sc, program, RC.nows(sc), RC.params(case))
    want = np.load(D.GOLDEN + "/ref_%s_%s.npz" % (program, case))
    assert sorted(got) == sorted(want.files)
    for k in got:
        assert np.array_equal(got[k], want[k]), "stale fixture: %s of ref_%s_%s" % (k, program, case)


@pytest.mark.parametrize("case", D.CASES)
@pytest.mark.parametrize("program", PROGRAMS)
def test_b_input_digest(program, case):
    fx = D.fixture(program, case)
    assert fx["params"] == RC.params(case)
    sc = D.scenario(case)
    assert R.input_digest(sc, program, RC.nows(sc)) == fx["input_sha"]
    assert len(fx["batches"]) == len(sc.batches)
    if case == "hand":
        assert sum(pk.n for pk in sc.batches) <= 200


@pytest.mark.parametrize("case", D.CASES)
@pytest.mark.parametrize("program", PROGRAMS)
def test_unmodelled_helper_count_is_zero(program, case):
    D.check_unmodelled(D.fixture(program, case))


def oracle_events(sink, out, frames, ran, stride):
    """The oracle's records of a batch in emission order with their packet: trace records as
    the sink captured them, header and payload.  o_ingress_events emits a drop record's 32-byte
    header only, no captured bytes: the payload compared here is filled in from the oracle's
    final frame, so for ingress drops the oracle's own output under test is the header."""
    recs, own = [], []
    for i in range(len(out)):
        if not ran[i]:
            continue                  # the caller's drop notification: that program is not run here
        for k in range(int(sink.cnt[i])):
            r = sink.ev[i, k].copy()
            if r[0] == 1:
                cap = min(int(r[12:16].view("<u4")[0]), stride)
                r[32:32 + cap] = frames[i, :cap]
            recs.append(r)
            own.append(i)
    return np.array(recs, np.uint8).reshape(-1, 160), np.array(own, np.int64)


@pytest.mark.parametrize("case", D.CASES)
def test_c_oracle_handle_policy(case):
    fx = D.fixture("lxc", case)
    sc = D.scenario(case)
    ref = OracleDP(sc)
    for b, pk, now in zip(fx["batches"], sc.batches, RC.nows(sc)):
        with O.TraceSink(pk.n) as sink:
            out, frames = ref.ingress_frames(pk, now)
            ref.ingress_events(pk, out)
        _, ev, own = D.check_ingress_batch(b, pk, sc, out, frames)
        ran = b["obs"]["ret"] != R.NOT_RUN
        assert np.all((out["action"][~ran] == 2) & (out["reason"][~ran] == R.DROP_MISSED_TAIL_CALL))
        oev, oown = oracle_events(sink, out, frames, ran, pk.frames.shape[1])
        assert np.array_equal(own, oown), "events come from other packets than in the reference"
        assert np.array_equal(ev, oev), "event bytes differ from the reference"
        for name in fx["maps"]:
            assert ref.dump(name) == D.dump_dict(b["maps"][name]), "map %s differs from the reference" % name


def test_hand_case_reaches_what_it_is_built_for():
    D.check_hand_expectations(D.fixture("lxc", "hand"), D.scenario("hand"))


@pytest.mark.parametrize("case", D.CASES)
def test_c_oracle_lb(case):
    fx = D.fixture("lb", case)
    sc = D.scenario(case)
    ref = OracleDP(sc)
    model = LM.LbFramesModel(sc)
    for b, pk in zip(fx["batches"], sc.batches):
        out, nd6 = ref.lb(pk)
        recs, mnd6, frames = model.batch(pk)
        assert np.array_equal(recs, out) and np.array_equal(mnd6, nd6)
        D.check_lb_batch(b, pk, out, nd6, frames)
        ev, own = D.lb_events_want(b, pk)
        assert np.array_equal(own, np.nonzero(out["action"] == 2)[0])
        assert np.array_equal(ev, LM.drop_events(pk, recs, frames)), "LB drop events differ from the reference"


# ---- (d) the shim's checksum helpers against a big-integer fold --------------------------
def fold(x):
    """RFC 1071: an arbitrary-size one's-complement sum folded to 16 bits."""
    while x >> 16:
        x = (x & 0xffff) + (x >> 16)
    return x


def words16(b):
    return sum(int.from_bytes(b[i:i + 2], "little") for i in range(0, len(b), 2))


def expect_replace(hc, frm, to, size, l4, flags):
    """RFC 1624 eqn. 3 on integers; returns (ret, new checksum word)."""
    EINVAL = -22
    mm0 = l4 and flags & 0x20
    if mm0 and not flags & 0x40 and hc == 0:    # "no checksum" is left alone, before the size is looked at
        return 0, hc
    if size == 0:
        if frm:
            return EINVAL, hc
    elif size == 2:
        frm, to = frm & 0xffff, to & 0xffff
    elif size != 4:
        return EINVAL, hc
    s = (~hc & 0xffff) + ((~frm & 0xffffffff) if size else 0xffffffff) + to
    new = ~fold(s) & 0xffff
    if mm0 and new == 0:
        new = 0xffff
    return 0, new


@pytest.mark.parametrize("op", [0, 1, 2])
def test_d_shim_checksum_helpers(op):
    if not R.has_runner():
        pytest.skip("oracle/_ref/ absent: no reference checkout on this machine")
    rng = random.Random(0xC5 + op)
    recs, want = [], []
    for i in range(1000):
        buf = bytearray(rng.randbytes(64))
        if op == 0:
            fs, ts = rng.choice([0, 4, 8, 16, 32]), rng.choice([0, 4, 8, 16, 32])
            if i % 10 == 0:
                fs = rng.choice([1, 2, 3, 5, 7, 15])                  # odd sizes: -EINVAL
            if i % 10 == 1:
                buf[32:64] = buf[0:32]                                # to == from: a zero result
                ts = fs
            seed = rng.choice([0, rng.getrandbits(32)])
            recs.append((0, fs, ts, seed, 0, buf))
            if fs % 4 or ts % 4:
                want.append(None)
            else:
                frm = sum((~int.from_bytes(buf[k:k + 4], "little")) & 0xffffffff for k in range(0, fs, 4))
                to = sum(int.from_bytes(buf[32 + k:32 + k + 4], "little") for k in range(0, ts, 4))
                want.append(fold(seed + frm + to))
        else:
            off = rng.randrange(0, 62, 2)
            size = rng.choice([0, 2, 4, 4, 2, 0, 1, 3]) if i % 8 == 0 else rng.choice([0, 2, 4])
            frm, to = rng.getrandbits(32), rng.getrandbits(32)
            if size == 0 and i % 16:
                frm = 0
            flags = size
            if op == 2:
                flags |= rng.choice([0, 0x10, 0x20, 0x30, 0x60])
                if i % 7 == 0:
                    buf[off:off + 2] = b"\0\0"                         # a UDP checksum of 0
            if i % 9 == 0:                                             # force a zero result: HC' = 0 <=> ~HC + ~m + m' = 0xffff
                frm, size, flags = 0, 0, flags & ~0xf
                hc = int.from_bytes(buf[off:off + 2], "little")
                to = hc                                                # ~hc + 0xffffffff + hc folds to 0xffff
            if i % 50 == 3:
                off = 63                                               # odd offset / past the end
            if i % 50 == 7:
                off = rng.randrange(1, 61, 2)                          # odd offset inside the packet
            recs.append((op, off, frm, to, flags, buf))
            hc = int.from_bytes(buf[off:off + 2], "little")
            if off + 2 > 64 or off & 1:
                want.append((-14, None))
            else:
                want.append(expect_replace(hc, frm, to, flags & 0xf, op == 2, flags))
    got = R.csum_run(recs)
    zero = 0
    for (ret, out), rec, w in zip(got, recs, want):
        buf = rec[5]
        if op == 0:
            if w is None:
                assert ret == -22
            else:
                assert fold(ret & 0xffffffff) % 0xffff == w % 0xffff, rec[:5]
                zero += w % 0xffff == 0
            assert out == bytes(buf)
        else:
            wret, whc = w
            assert ret == wret, rec[:5]
            exp = bytearray(buf)
            if wret == 0:
                exp[rec[1]:rec[1] + 2] = whc.to_bytes(2, "little")
                zero += whc in (0, 0xffff)
            assert out == bytes(exp), rec[:5]
    assert zero > 20, "the zero-result cases did not occur"
