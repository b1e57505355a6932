"""Bit-exact parity at the configurations' real table shapes (BASELINE configs 2
and 5): the device stream of the bench, checked against the oracle on a
flow-group sample (whole address pairs, so the sampled run of the stateful path
is exact) — every sampled record and, after the last step, every CT entry of the
sampled pairs."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from cilium_amd import synth, stream
from cilium_amd.datapath import Datapath, ING_OUT, PIPE_OUT
from cilium_amd.synth import Packets
from oracle.scenario import OracleDP
from oracle import parity as PY


@pytest.fixture(scope="module", autouse=True)
def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(0)


class _Cols:
    def __init__(self, cols, n):
        from cilium_amd.datapath import DeviceBatch
        self.n, self.device, self.cdict = n, "cuda", cols
        self.saddr6 = self.daddr6 = self.flow_hash = None
        for k, v in cols.items():
            setattr(self, k, v)
        self._cols = DeviceBatch.cols

    def cols(self):
        return self._cols(self)


def _host_packets(cdict, idx):
    c = {k: v[idx].cpu().numpy() for k, v in cdict.items()}
    to_u = {np.dtype(np.int32): np.uint32, np.dtype(np.int16): np.uint16}
    c = {k: (v.view(to_u[v.dtype]) if v.dtype in to_u else v) for k, v in c.items()}
    f, lens = stream.to_frames(c)
    return Packets(f, lens, c["src_identity"], c["ifindex"], c["lxc_id"], c["tc_index"])


def test_config2_real_shape_sampled_parity():
    """Config 2 at its real table shape: 256 endpoints, 4,352 identities, full-size
    per-endpoint policy (2,000 L3 + 4,000 L4 + 32 wildcard entries) and CIDR maps,
    2^20 address pairs; the bench's steady-state stream (1M packets per step, 4
    steps) with its pre-inserted egress replies.  1/8 of the pairs through the
    oracle: records and the sampled pairs' CT entries bit-exact."""
    sc, P, _ = synth.config2_tables(n_pairs=1 << 20, ct_max=1 << 24)
    st = stream.Stream(P, flows_per_step=1 << 18, device="cuda")
    S0, N = 3, 4
    rk, rv = st.reply_ct_entries(S0 + N)
    sc.maps["cilium_ct4_global"].keys, sc.maps["cilium_ct4_global"].vals = rk, rv
    dp, ref = Datapath(sc, pin_prefix=None), OracleDP(sc, shards=8)
    div = 8
    samp = torch.from_numpy(PY.pair_sampled(st.p_saddr.cpu().numpy(), st.p_daddr.cpu().numpy(), div)).cuda()
    compared = 0
    for s in range(N):
        cols, p, n = st.step(S0 + s)
        b = _Cols(cols, n)
        out = dp.ingress(b, sc.now + s)
        torch.cuda.synchronize()
        idx = torch.nonzero(samp[p]).squeeze(1)
        r = ref.ingress(_host_packets(cols, idx), sc.now + s, threads=8)
        g = out[idx].cpu().numpy().view(ING_OUT).ravel()
        bad, first = PY.compare_records(g, r)
        assert bad == 0, f"step {s}: {bad} mismatches, first sampled row {first}: gpu={g[first]} ref={r[first]}"
        compared += len(r)
    assert compared > 400_000
    assert len(np.unique(r["ct_ret"])) == 4 and (r["action"] == 2).any() and (r["action"] == 7).any()
    gk, gv, gtot = PY.gpu_table_sampled(dp.fd["cilium_ct4_global"], 14, 48, div)
    ok, ov = PY.oracle_table_sampled(ref.m["cilium_ct4_global"], div)
    n, bad = PY.compare_tables(gk, gv, ok, ov)
    assert bad == 0 and n > 100_000, (n, bad, gtot)


def test_config5_real_shape_parity_with_eviction():
    """Config 5 at its real table shape: v6_fix 100k /128s and v6_dyn 10k /32-/127
    prefixes through bpf_xdp's check_v6, bpf_netdev's handle_ipv6 (flow-label
    identities), ipv6_policy / ct_lookup6 on a 10,485,760-entry LRU CT pre-filled
    past its low watermark, so the LRU stand-in evicts at full scale after every
    batch.  The whole stream (262k packets per step) through the oracle: records,
    the eviction logs and the full CT6 bit-exact."""
    from cilium_amd import bpf
    from cilium_amd._lib import lib, gf_ct_evict_rec
    sc, P, meta = synth.config5_tables(n_pairs=1 << 20, prefill=10_300_000)
    st = stream.Stream6Frames(P, meta, flows_per_step=1 << 16, device="cuda")
    S0, N = 3, 4
    rk, rv = st.reply_ct6_entries(S0 + N)
    ct6 = sc.maps["cilium_ct6_global"]
    ct6.keys, ct6.vals = synth.ct6_prefill(meta, rk, rv, sc.now)
    dp, ref = Datapath(sc, pin_prefix=None), OracleDP(sc, shards=8)
    for s in range(N):
        f, lens, p = st.step(S0 + s)

        class B:
            pass
        b = B()
        b.frames, b.len, b.tc_index, b.flow_hash, b.n, b.device = f, lens, None, None, f.shape[0], "cuda"
        out, _, _ = dp.pipeline(b, sc.now + s, snap_out=False)
        torch.cuda.synchronize()
        r = ref.pipeline(Packets(f.cpu().numpy(), lens.cpu().numpy().view(np.uint32)), sc.now + s, threads=8)[0]
        g = out.cpu().numpy().view(PIPE_OUT).ravel()
        bad, first = PY.compare_records(g, r)
        assert bad == 0, f"step {s}: {bad} mismatches, first row {first}: gpu={g[first]} ref={r[first]}"
        assert bpf.GetMapInfo(dp.fd["cilium_ct6_global"]).Entries == ref.m["cilium_ct6_global"].count() <= 10_485_760
    assert set(np.unique(r["stage"])) >= {1, 4} and len(np.unique(r["ct_ret"][r["stage"] == 4])) >= 3
    recs = (gf_ct_evict_rec * 64)()
    nlog = lib.gf_ct_evict_log(dp.fd["cilium_ct6_global"], recs, 64)
    glog = [(x.seq, x.now_sec, x.age_cut, x.hand_line, x.lines, x.evicted) for x in recs[:nlog]]
    assert glog == ref.lru_log["cilium_ct6_global"] and len(glog) >= 1
    m = bpf.Map("ct6", 9, 40, 48, 10_485_760)
    m.fd = dp.fd["cilium_ct6_global"]
    gk, gv = m.DumpArrays()
    ok, ov = ref.m["cilium_ct6_global"].dump_arrays()
    n, bad = PY.compare_tables(gk, gv, ok, ov)
    assert bad == 0 and n > 9_000_000, (n, bad)


def test_config3_real_shape():
    """Config 3 at its real table shape: bpf_lb over 100,000 services (90% VIP:port,
    10% L3-only) and ~1,000,000 backend slots in one 2M-entry lbmap (the
    AddSVC2BPFMap population of pkg/maps/lbmap/lbmap.go:320-371), 100k revNAT
    entries; 2M packets (85% Zipf-1.1 VIP traffic, 5% L3-only VIPs on random ports,
    10% non-service).  The whole batch against the oracle (lb.h:566-613 lookups,
    slave = hash % count + 1, the lb4_xlate fields), plus the counter block."""
    import ctypes as C
    from cilium_amd._lib import lib
    from cilium_amd.datapath import DeviceBatch, LB_OUT, to_numpy
    sc = synth.config3(n_packets=2_000_000)
    assert sc.maps["cilium_lb4_services"].n() > 1_000_000
    dp, ref = Datapath(sc, pin_prefix=None), OracleDP(sc)
    pk = sc.batches[0]
    cnt = torch.zeros(512, dtype=torch.int64, device="cuda")
    lib.gf_set_stats_sink(C.c_void_p(cnt.data_ptr()))
    try:
        lo, _ = dp.lb(DeviceBatch(pk, with_v6=False))
        torch.cuda.synchronize()
    finally:
        lib.gf_set_stats_sink(None)
    g = to_numpy(lo, LB_OUT)
    r, _ = ref.lb(pk, threads=8)
    bad, first = PY.compare_records(g, r)
    assert bad == 0, f"{bad} mismatches, first {first}: gpu={g[first]} ref={r[first]}"
    # every outcome of the path is exercised at this shape
    assert (r["action"] == 7).mean() > 0.8 and (r["reason"] == 158).sum() == 0
    assert (r["new_dport"] != 0).any() and len(np.unique(r["slave"])) >= 19
    c = cnt.cpu().numpy()
    assert c[268] == pk.n and c[269] == np.asarray(pk.lens, np.int64).sum()
    for a in np.unique(r["action"]):
        assert c[256 + int(a)] == (r["action"] == a).sum(), f"action {a}"
    for x in range(1, 256):
        assert c[x] == (r["reason"] == x).sum(), f"reason {x}"


def test_config4_real_shape_sampled():
    """Config 4 at its real table shape: config 2's endpoints, policies and CIDR maps
    over 2^20 address pairs, config 1's prefilter (10k LPM prefixes + 2k /32s),
    config 3's service population (100k services / ~1M backends) next to the
    endpoints' own VIPs, composed bpf_xdp -> bpf_lb -> bpf_netdev -> handle_policy
    over raw frames of the bench's steady-state stream (4 steps of 1M frames, 30% of
    the pairs addressed through a VIP).  1/8 of the post-LB address pairs through the
    oracle: pipeline records and rewritten frames of every sampled packet, then the
    sampled pairs' CT entries, bit-exact."""
    sc, P, vip = synth.config4_tables(n_pairs=1 << 20, ct_max=1 << 24)
    assert sc.maps["cilium_lb4_services"].n() > 1_000_000
    st = stream.Stream(P, flows_per_step=1 << 18, device="cuda", vip_ip=vip)
    S0, N = 3, 4
    rk, rv = st.reply_ct_entries(S0 + N)
    sc.maps["cilium_ct4_global"].keys, sc.maps["cilium_ct4_global"].vals = rk, rv
    dp, ref = Datapath(sc, pin_prefix=None), OracleDP(sc, shards=8)
    div = 8
    samp = torch.from_numpy(PY.pair_sampled(st.p_saddr.cpu().numpy(), st.p_daddr.cpu().numpy(), div)).cuda()
    compared, stages, rets = 0, set(), set()
    for s in range(N):
        cols, p, n = st.step(S0 + s)
        f, lens = stream.device_frames(cols)

        class B:
            pass
        b = B()
        b.frames, b.len, b.tc_index, b.flow_hash, b.n, b.device = f, lens, cols["tc_index"], None, n, "cuda"
        out, _, snap = dp.pipeline(b, sc.now + s, snap_out=True)
        torch.cuda.synchronize()
        idx = torch.nonzero(samp[p]).squeeze(1)
        pk = Packets(f[idx].cpu().numpy(), lens[idx].cpu().numpy().view(np.uint32),
                     tc_index=cols["tc_index"][idx].cpu().numpy())
        ro, _, rs = ref.pipeline(pk, sc.now + s, threads=8)
        g = out[idx].cpu().numpy().view(PIPE_OUT).ravel()
        bad, first = PY.compare_records(g, ro)
        assert bad == 0, f"step {s}: {bad} mismatches, first sampled row {first}: gpu={g[first]} ref={ro[first]}"
        gs = snap[idx].cpu().numpy()
        bad_f = np.nonzero((gs != rs).any(axis=1))[0]
        if len(bad_f):
            det = []
            for j in bad_f[:4]:
                offs = np.nonzero(gs[j] != rs[j])[0]
                det.append(f"row {j} rec={ro[j]} len={pk.lens[j]} offs={offs.tolist()} gpu={gs[j][offs].tolist()} "
                           f"ref={rs[j][offs].tolist()} in={pk.frames[j][offs].tolist()} frame={pk.frames[j][:64].tolist()}")
            raise AssertionError(f"step {s}: {len(bad_f)} rewritten frames differ:\n" + "\n".join(det))
        compared += len(ro)
        stages |= set(np.unique(ro["stage"]).tolist())
        rets |= set(np.unique(ro["ct_ret"][ro["stage"] == 4]).tolist())
    assert compared > 400_000
    assert {1, 4} <= stages and len(rets) == 4, (stages, rets)
    gk, gv, gtot = PY.gpu_table_sampled(dp.fd["cilium_ct4_global"], 14, 48, div)
    ok, ov = PY.oracle_table_sampled(ref.m["cilium_ct4_global"], div)
    n, bad = PY.compare_tables(gk, gv, ok, ov)
    assert bad == 0 and n > 100_000, (n, bad, gtot)


def test_reply_ct_entries_on_the_device_equal_the_cpu_build():
    """Stream.reply_ct_entries sorts and de-duplicates on the stream's device: on the
    GPU it must give the rows the CPU device gives (which tests/test_bench_launcher.py
    pins to the host construction), in the same order; few pairs, so most keys repeat,
    and more than one 16-step block."""
    sc, P, _ = synth.config2_tables(n_pairs=256, ct_max=65536, n_ep=16, n_ids=256, n_l3=64, n_l4=128, n_wc=8,
                                    n_cidr=16)
    gk, gv = stream.Stream(P, flows_per_step=1 << 14, device="cuda").reply_ct_entries(21)
    ck, cv = stream.Stream(P, flows_per_step=1 << 14, device="cpu").reply_ct_entries(21)
    assert len(ck) > 10_000 and np.array_equal(gk, ck) and np.array_equal(gv, cv)
