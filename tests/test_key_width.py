"""The flow-group bucket key follows the batch size (gf_key_bits, gf_common.h):
9 bits up to 64 packets, 18 up to 2^15, 27 up to 2^24, 32 above (the frame entry
points: 32 above 2^15).  Narrow keys make flow groups
share buckets and move the family bit and the skip value, so these batches put
the device against the oracle byte for byte (records, CT entries, policy
counters) exactly where a narrow key could go wrong."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from cilium_amd import synth
from cilium_amd.synth import ICMP, TCP, UDP, F_ACK, F_SYN, ip4

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cilium_amd", "csrc")


# ---- the width rule and the group hash, restated (checked against the C code below)
SIZES = (0, 2, 64, 65, 4096, 1 << 15, (1 << 15) + 1, 1 << 24, (1 << 24) + 1, 1 << 30)


def key_bits(n, radix=9, wide=False):
    """wide: the frame entry points (pipeline, overlay, host) skip the three-pass tier."""
    lg = 1
    while (1 << lg) < n:
        lg += 1
    passes = min(4, -(-(lg + 3) // radix))
    if wide and passes > 2:
        passes = 4
    return min(32, radix * passes)


def _rotl(x, r):
    return (x << np.uint32(r)) | (x >> np.uint32(32 - r))


def hash_words(words, nbytes):
    """gf_hash_words over columns of u32 words."""
    h = np.full(np.shape(words[0]), 0x9747b28c ^ nbytes, np.uint32)
    with np.errstate(over="ignore"):
        for w in words:
            k = _rotl(np.asarray(w, np.uint32) * np.uint32(0xcc9e2d51), 15) * np.uint32(0x1b873593)
            h = _rotl(h ^ k, 13) * np.uint32(5) + np.uint32(0xe6546b64)
        h ^= h >> np.uint32(16)
        h *= np.uint32(0x85ebca6b)
        h ^= h >> np.uint32(13)
        h *= np.uint32(0xc2b2ae35)
        h ^= h >> np.uint32(16)
    return h


def pair_hash4(a, b):
    """gf_pair_hash4 of two addresses as the parser loads them (the wire bytes as a LE word)."""
    a, b = np.asarray(a, np.uint32), np.asarray(b, np.uint32)
    return hash_words([np.minimum(a, b), np.maximum(a, b)], 8)


def wire(a):
    return np.asarray(a, np.uint32).byteswap()


# Found on the CPU by a birthday search over (remote 10.128.4.0/20, endpoint 10.1.0.1-12):
# two address pairs whose pair hashes agree in their low 17 bits (the 18-bit key of a
# 4,096-packet batch), and a pair whose low 17 hash bits are all ones (the skip value).
PAIR_A = (ip4("10.128.7.252"), ip4("10.1.0.3"))      # gf_pair_hash4 0xd5ba004a
PAIR_B = (ip4("10.128.13.108"), ip4("10.1.0.10"))    # gf_pair_hash4 0x58ce004a
PAIR_SKIP = (ip4("10.129.99.13"), ip4("10.1.0.5"))   # gf_pair_hash4 0x6de7ffff
EP0 = ip4("10.1.0.1")                                 # synth.fuzz: endpoint e is EP0 + e, lxc_id 2000 + e


def test_width_rule_and_hard_coded_pairs():
    assert [key_bits(n) for n in SIZES] == \
        [9, 9, 9, 18, 18, 18, 27, 27, 32, 32]
    assert [key_bits(n, wide=True) for n in SIZES] == [9, 9, 9, 18, 18, 18, 32, 32, 32, 32]
    ha, hb = int(pair_hash4(wire(PAIR_A[0]), wire(PAIR_A[1]))), int(pair_hash4(wire(PAIR_B[0]), wire(PAIR_B[1])))
    m17 = (1 << (key_bits(4096) - 1)) - 1
    assert PAIR_A != PAIR_B and ha != hb and (ha & m17) == (hb & m17)
    assert int(pair_hash4(wire(PAIR_SKIP[0]), wire(PAIR_SKIP[1]))) & m17 == m17


_PROBE = r"""
#include "gf_common.h"
#include <stdio.h>
int main() {
    const uint32_t ns[] = {0u, 2u, 64u, 65u, 4096u, 1u << 15, (1u << 15) + 1u, 1u << 24, (1u << 24) + 1u, 1u << 30};
    for (uint32_t n : ns) { gf_key_cfg K = gf_key_for(n); printf("%u %u %u ", K.bits, K.fam, K.hash); }
    for (uint32_t n : ns) printf("%u ", gf_key_for(n, true).bits);
    printf("\n%u %u %u\n", gf_pair_hash4(0xfc07800au, 0x0300010au), gf_pair_hash4(0x6c0d800au, 0x0a00010au),
           gf_pair_hash4(0x0d63810au, 0x0500010au));
    return 0;
}
"""


def _probe(tmp_path, *flags):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or shutil.which("hipcc")
    assert cxx, "no host C++ compiler"
    src, exe = tmp_path / "probe.cpp", tmp_path / ("probe" + "".join(flags).replace("=", "_"))
    src.write_text(_PROBE)
    subprocess.run([cxx, "-std=c++17", "-O1", "-I", CSRC, *flags, str(src), "-o", str(exe)], check=True)
    a, b = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.strip().split("\n")
    return [int(x) for x in a.split()], [int(x) for x in b.split()]


def test_rule_function_and_forced_width(tmp_path):
    """The host code's own rule (gf_key_for) equals the restatement, its group hash
    equals the numpy one on the hard-coded pairs, and GF_KEY_BITS=32 forces 32 bits
    for every batch size (the A/B build of the former fixed key)."""
    cfg, hs = _probe(tmp_path)
    want = []
    for n in SIZES:
        b = key_bits(n)
        want += [b, 1 << (b - 1), (1 << (b - 1)) - 1]
    k = 3 * len(SIZES)
    assert cfg[:k] == want and cfg[k:] == [key_bits(n, wide=True) for n in SIZES]
    assert hs == [int(pair_hash4(wire(p[0]), wire(p[1]))) for p in (PAIR_A, PAIR_B, PAIR_SKIP)]
    assert int(wire(PAIR_A[0])) == 0xfc07800a and int(wire(PAIR_SKIP[1])) == 0x0500010a
    cfg32, _ = _probe(tmp_path, "-DGF_KEY_BITS=32")
    assert cfg32 == [32, 1 << 31, (1 << 31) - 1] * len(SIZES) + [32] * len(SIZES)
    cfg8, _ = _probe(tmp_path, "-DGF_SORT_RADIX=8")
    assert cfg8[:k:3] == [key_bits(n, 8) for n in SIZES]


# ---- batches
def _allowed_identity(sc, e):
    """An identity with an L3 entry in endpoint e's policy map (new flows are let in)."""
    k = sc.maps[f"pol{e}"].keys
    l3 = k[(k[:, 4:8] == 0).all(axis=1)]
    ids = l3[:, :4].copy().view("<u4").reshape(-1)
    return int(ids[ids != 0][0])


def _reply_entries(sc, pairs, sport, dport):
    """Egress-style CT entries (endpoint -> remote), so that remote:sport -> endpoint:dport is a reply."""
    ct = sc.maps["ct4"]
    E = np.array([p[1] for p in pairs], np.uint32)
    R = np.array([p[0] for p in pairs], np.uint32)
    n = len(pairs)
    k = synth.ct4_keys(E, R, synth.raw16(np.full(n, sport)), synth.raw16(np.full(n, dport)), np.full(n, TCP), np.zeros(n))
    v = synth.ct_vals(n, 4000, 0, 0, 300, tx=(3, 300))
    ct.keys, ct.vals = synth.dedup(np.concatenate([ct.keys, k]), np.concatenate([ct.vals, v]))


def _group_rows(sc, pair, stride, rounds):
    """One flow group's packets, remote -> endpoint: per round a new TCP flow, an
    established packet of it, the reply to a pre-inserted egress entry, a new UDP
    flow; once, after the first flow exists, an ICMP error (destination unreachable)
    in the same direction: it hits the related entry that flow's ct_create4 wrote in
    this batch (the lane's related-entry cache) and so is CT_ESTABLISHED, not CT_NEW."""
    R, E = pair
    e = E - EP0
    sp, dp, pr, tf, it = [], [], [], [], []
    for r in range(rounds):
        sp += [30000 + r, 30000 + r, 41000, 31000 + r]
        dp += [80, 80, 8080, 53]
        pr += [TCP, TCP, TCP, UDP]
        tf += [F_SYN, F_ACK, F_ACK, 0]
        it += [0, 0, 0, 0]
        if r == 0:
            sp.append(0); dp.append(0); pr.append(ICMP); tf.append(0); it.append(3)
    n = len(sp)
    f, lens = synth.frames_v4(n, stride, R, E, pr, sp, dp, tf, it, 0, 5, payload=12)
    return f, lens, np.full(n, _allowed_identity(sc, e), np.uint32), np.full(n, 10 + e, np.uint32), \
        np.full(n, 2000 + e, np.uint16)


ICMP_ROW = 4                                            # the ICMP error's position in _group_rows' packets


def _put(pk, rows, f, lens, sid, ifx, lid):
    pk.frames[rows] = f
    pk.lens[rows] = lens
    pk.src_identity[rows], pk.ifindex[rows], pk.lxc_id[rows] = sid, ifx, lid
    pk.tc_index[rows] = 0


def shared_bucket_scenario():
    """4,096 packets (18-bit key): groups A and B share a bucket, their packets
    strictly interleaved (A, B, A, B, ...) in the middle of a fuzz batch."""
    sc = synth.fuzz(seed=21, n_packets=4096, n_batches=1)
    _reply_entries(sc, [PAIR_A, PAIR_B], 41000, 8080)
    pk = sc.batches[0]
    ga, gb = _group_rows(sc, PAIR_A, pk.frames.shape[1], 6), _group_rows(sc, PAIR_B, pk.frames.shape[1], 6)
    m = len(ga[1])
    ra, rb = 1000 + 2 * np.arange(m), 1001 + 2 * np.arange(m)
    _put(pk, ra, *ga)
    _put(pk, rb, *gb)
    return sc, ra, rb


def skip_key_scenario():
    """4,096 frames through the whole pipeline: a group whose masked pair hash is the
    skip value (all ones at 18 bits) among packets that end before the tail call."""
    sc = synth.pipeline_fuzz(seed=22, n_packets=4096, n_batches=1)
    # bpf_netdev derives the source identity itself: FIXED_SRC_SECCTX, one the group's endpoint lets in
    sc.netdev = dict(sc.netdev, flags=1, fixed_secctx=_allowed_identity(sc, PAIR_SKIP[1] - EP0))
    _reply_entries(sc, [PAIR_SKIP], 41000, 8080)
    pk = sc.batches[0]
    g = _group_rows(sc, PAIR_SKIP, pk.frames.shape[1], 6)
    g[0][:, 22] = 64                                    # TTL
    rows = 500 + 3 * np.arange(len(g[1]))
    _put(pk, rows, *g)
    return sc, rows


def mixed_boundary_scenario(n):
    """One IPv4 + IPv6 batch of n packets (synth.fuzz: 13 % IPv6 rows, both families reach conntrack)."""
    return synth.fuzz(seed=23, n_packets=n, n_batches=1)


def elephant_scenario():
    """One group of 3,000 packets among 1,096 single-packet groups (18-bit key)."""
    sc = synth.fuzz(seed=24, n_packets=4096, n_batches=1)
    pk = sc.batches[0]
    S = pk.frames.shape[1]
    rng = np.random.default_rng(24)
    big = np.sort(rng.choice(4096, 3000, replace=False))
    R, E = PAIR_A
    e = E - EP0
    k = np.arange(3000)
    f, lens = synth.frames_v4(3000, S, R, E, TCP, 20000 + k % 40, 80, np.where(k % 5 == 0, F_SYN, F_ACK), 0, 0, 5,
                              payload=k % 32)
    _put(pk, big, f, lens, np.full(3000, _allowed_identity(sc, e), np.uint32), np.full(3000, 10 + e, np.uint32),
         np.full(3000, 2000 + e, np.uint16))
    rest = np.setdiff1d(np.arange(4096), big)
    m = len(rest)
    j = np.arange(m)
    es = j % 10
    f, lens = synth.frames_v4(m, S, ip4("10.130.0.0") + j, EP0 + es, TCP, 1000 + j % 7, 80, F_SYN, 0, 0, 5, payload=4)
    sid = np.array([_allowed_identity(sc, int(x)) for x in range(10)], np.uint32)[es]
    _put(pk, rest, f, lens, sid, (10 + es).astype(np.uint32), (2000 + es).astype(np.uint16))
    return sc, big


# ---- the device against the oracle
gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(0)
    return torch


def _sync():
    import torch
    torch.cuda.synchronize()


def _cmp(a, b, what):
    if not np.array_equal(a, b):
        bad = np.nonzero(a != b)[0]
        raise AssertionError(f"{what}: {len(bad)} mismatches, first at {bad[0]}: gpu={a[bad[0]]} ref={b[bad[0]]}")


def _ingress_equals_oracle(sc):
    from cilium_amd.datapath import Datapath, DeviceBatch, ING_OUT, to_numpy
    from oracle.scenario import OracleDP
    dp, ref = Datapath(sc, pin_prefix=None), OracleDP(sc)
    pk = sc.batches[0]
    io = dp.ingress(DeviceBatch(pk), sc.now)
    _sync()
    want = ref.ingress(pk, sc.now)
    _cmp(to_numpy(io, ING_OUT), want, "ingress records")
    for name in ("ct4", "ct6"):
        assert dp.dump_map(name) == ref.dump(name), name
    for e in range(16):
        assert dp.dump_map(f"pol{e}") == ref.dump(f"pol{e}"), f"policy counters pol{e}"
    return want


def _kinds(rec, rows):
    return set(int(x) for x in rec["ct_ret"][rows][rec["action"][rows] != 2])


@gpu
def test_two_groups_in_one_bucket(dev):
    sc, ra, rb = shared_bucket_scenario()
    assert sc.batches[0].n == 4096 and key_bits(4096) == 18
    want = _ingress_equals_oracle(sc)
    # both groups: new, established and reply packets (CT_NEW 0, CT_ESTABLISHED 1, CT_REPLY 2), none dropped,
    # and the ICMP error found the related entry of the flow created two packets of its group earlier
    for rows in (ra, rb):
        assert _kinds(want, rows) == {0, 1, 2} and (want["action"][rows] != 2).all()
        assert want["ct_ret"][rows[ICMP_ROW]] == 1


def _pipeline_equals_oracle(sc):
    from cilium_amd.datapath import Datapath, DeviceBatch, PIPE_OUT, to_numpy
    from oracle.scenario import OracleDP
    dp, ref = Datapath(sc, pin_prefix=None), OracleDP(sc)
    pk = sc.batches[0]
    out, nd6, snap = dp.pipeline(DeviceBatch(pk, parse=False), sc.now)
    _sync()
    ro, rn6, rs = ref.pipeline(pk, sc.now)
    _cmp(to_numpy(out, PIPE_OUT), ro, "pipeline records")
    assert np.array_equal(nd6.cpu().numpy(), rn6)
    assert np.array_equal(snap.cpu().numpy(), rs), "rewritten frames"
    for name in ("ct4", "ct6", "cilium_proxy4", "cilium_proxy6"):
        assert dp.dump_map(name) == ref.dump(name), name
    for e in range(16):
        assert dp.dump_map(f"pol{e}") == ref.dump(f"pol{e}"), f"policy counters pol{e}"
    return ro


@gpu
def test_skip_valued_group_is_classified(dev):
    sc, rows = skip_key_scenario()
    assert key_bits(sc.batches[0].n, wide=True) == 18    # the pipeline's width at 4,096 frames
    ro = _pipeline_equals_oracle(sc)
    # the group reached handle_policy (stage 4) and its flows were created; others ended before the tail call
    assert (ro["stage"][rows] == 4).all() and _kinds(ro, rows) == {0, 1, 2} and ro["ct_ret"][rows[ICMP_ROW]] == 1
    assert (ro["stage"] != 4).sum() > 100


@gpu
def test_pipeline_above_two_pass_tier_keeps_32_bits(dev):
    """One frame past 2^15 the frame entry points go to the 32-bit key (rocPRIM's
    default sort config), not to 27 bits: front, skip run and schedule agree on it."""
    n = (1 << 15) + 1
    assert key_bits(n, wide=True) == 32 and key_bits(n) == 27
    ro = _pipeline_equals_oracle(synth.pipeline_fuzz(seed=25, n_packets=n, n_batches=1))
    assert (ro["stage"] == 4).sum() > n // 10 and (ro["stage"] != 4).sum() > n // 10


@gpu
@pytest.mark.parametrize("n", [1 << 15, (1 << 15) + 1])
def test_width_boundary_mixed_families(dev, n):
    """Two passes (18 bits) at 2^15 packets, three (27 bits) one packet above: the
    family bit moves from bit 17 to bit 26 and still sorts IPv6 groups after IPv4."""
    assert key_bits(n) == (18 if n == 1 << 15 else 27)
    sc = mixed_boundary_scenario(n)
    want = _ingress_equals_oracle(sc)
    f = sc.batches[0].frames
    v6 = (f[:, 12] == 0x86) & (f[:, 13] == 0xdd)
    assert v6.sum() > n // 20 and (~v6).sum() > n // 2
    assert (want["ct_ret"][v6] != 0).any() or (want["action"][v6] != 2).any()


@gpu
def test_elephant_group_at_two_pass_width(dev):
    sc, big = elephant_scenario()
    assert len(big) == 3000 and sc.batches[0].n - len(big) == 1096 and key_bits(4096) == 18
    want = _ingress_equals_oracle(sc)
    assert _kinds(want, big) >= {0, 1}
