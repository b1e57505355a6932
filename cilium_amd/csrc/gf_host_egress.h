// gf_host_egress.h — gf_lxc_egress_classify on the host: EgWs, k_eg_init, the connection-group
// schedule and hazard check, egress_call, and the handle_policy pass over the local deliveries
// (included by gf_kernels.hip after gf_map_bulk.h; it launches the k_eg_* / k_hz_* / k_ctlog_*
// kernels and runs the flow-group schedule and ingress_run of the handle_policy pass, over
// gf_host_ctx.h's contexts).

// ---- endpoint egress (from-container) ----
namespace {
struct EgWs { DevBuf erec, rec2, key2, seq, ctlog, ctlog_n, snap, ckey, s6, d6,
             hzk, hzfl, hztk, hztf, hzak, hzaf, hzst, vip4, vip6, keysP, key2P, rlog, rlog_n, v6blk,
             rsslot, rslist;
             uint32_t hz_gen = 0, hz_cap = 0;
             uint32_t *h_hz = nullptr;          // pinned: the ordering check's words, read back without a stream sync
             hipEvent_t ev_hz = nullptr;
             std::vector<std::pair<const Map *, uint64_t>> vip_stamp;
             uint32_t vip4_mask = 0, vip6_mask = 0; bool vip4_any = false, vip6_any = false; };
EgWs &eg_ws() { static const char tag = 0; return cur_ctx().get<EgWs>(&tag); }
}  // namespace

static int egress_ordered(const std::shared_ptr<PolicyArray> &a, const gf_lxc_batch *b, uint32_t now_sec,
                          gf_egress_out *out, uint8_t *snap_out, hipStream_t s, bool lru, uint32_t first, uint32_t depth);
static int egress_runs(const std::shared_ptr<PolicyArray> &a, const gf_lxc_batch *b, uint32_t now_sec,
                       gf_egress_out *out, uint8_t *snap_out, hipStream_t s, bool lru, const std::vector<uint32_t> &cut);
static int egress_each(const std::shared_ptr<PolicyArray> &a, const gf_lxc_batch *b, uint32_t now_sec,
                       gf_egress_out *out, uint8_t *snap_out, hipStream_t s, bool lru) {
    std::vector<uint32_t> cut(b->frames.n + 1);
    for (uint32_t j = 0; j <= b->frames.n; j++) cut[j] = j;
    return egress_runs(a, b, now_sec, out, snap_out, s, lru, cut);
}
// The rev-NAT addresses of the programs' revNAT maps as device sets (the ordering
// check's GF_HZ_VIP), rebuilt when a map changed through the API.
static int vip_sets(const std::vector<std::shared_ptr<ProgLxc>> &progs, EgWs &ew, hipStream_t s) {
    std::vector<std::pair<const Map *, uint64_t>> stamp;
    std::vector<Map *> m4, m6;
    for (auto &p : progs) {
        if (p->revnat4 && std::find(m4.begin(), m4.end(), p->revnat4.get()) == m4.end()) m4.push_back(p->revnat4.get());
        if (p->revnat6 && std::find(m6.begin(), m6.end(), p->revnat6.get()) == m6.end()) m6.push_back(p->revnat6.get());
    }
    for (Map *m : m4) stamp.push_back({m, m->host_gen * 2});
    for (Map *m : m6) stamp.push_back({m, m->host_gen * 2 + 1});
    if (stamp == ew.vip_stamp) return 0;                // (no maps and nothing built compare equal too)
    std::vector<uint32_t> a4;
    std::vector<std::array<uint32_t, 4>> a6;
    std::vector<uint8_t> v(32);
    for (int fam = 4; fam <= 6; fam += 2) {
        for (Map *m : fam == 4 ? m4 : m6) {
            std::lock_guard<std::recursive_mutex> g(m->mu);
            int r = m->pull();
            if (r) return r;
            for (uint64_t i = 0; i < m->ht.nslots; i++) {
                if (m->ht.state(i) != GF_SLOT_FULL) continue;
                m->ht.get_val(i, v.data());
                if (fam == 4) { uint32_t x; memcpy(&x, v.data(), 4); if (x) a4.push_back(x); }
                else { std::array<uint32_t, 4> x; memcpy(x.data(), v.data(), 16); if (x[0] | x[1] | x[2] | x[3]) a6.push_back(x); }
            }
        }
    }
    auto build = [&](size_t cnt, uint32_t &mask) { mask = 15; while ((uint64_t)mask + 1 < 4ull * cnt) mask = mask * 2 + 1; };
    ew.vip4_any = !a4.empty(); ew.vip6_any = !a6.empty();
    if (ew.vip4_any) {
        build(a4.size(), ew.vip4_mask);
        std::vector<uint32_t> t(ew.vip4_mask + 1, 0);
        for (uint32_t x : a4) {
            uint32_t slot = vip_slot(x) & ew.vip4_mask;
            while (t[slot] && t[slot] != x) slot = (slot + 1u) & ew.vip4_mask;
            t[slot] = x;
        }
        if (ew.vip4.ensure(t.size() * 4) ||
            hip_ok(hipMemcpyAsync(ew.vip4.p, t.data(), t.size() * 4, hipMemcpyHostToDevice, s), "vip4") ||
            hip_ok(hipStreamSynchronize(s), "vip4 sync"))
            return -EIO;
    }
    if (ew.vip6_any) {
        build(a6.size(), ew.vip6_mask);
        std::vector<std::array<uint32_t, 4>> t(ew.vip6_mask + 1, std::array<uint32_t, 4>{0, 0, 0, 0});
        for (auto &x : a6) {
            uint32_t slot = vip_slot(x[0] ^ vip_slot(x[1] ^ vip_slot(x[2] ^ vip_slot(x[3])))) & ew.vip6_mask;
            while ((t[slot][0] | t[slot][1] | t[slot][2] | t[slot][3]) && t[slot] != x) slot = (slot + 1u) & ew.vip6_mask;
            t[slot] = x;
        }
        if (ew.vip6.ensure(t.size() * 16) ||
            hip_ok(hipMemcpyAsync(ew.vip6.p, t.data(), t.size() * 16, hipMemcpyHostToDevice, s), "vip6") ||
            hip_ok(hipStreamSynchronize(s), "vip6 sync"))
            return -EIO;
    }
    ew.vip_stamp = stamp;
    return 0;
}
// The per-call words of egress_call in one launch instead of four fills: the
// sequence words (seq[1] the ordering check's flag, seq[3] its first hazard,
// ~0 = none), both log counts and the front's scratch counter block.
__global__ __launch_bounds__(256) void k_eg_init(uint32_t *seq, uint32_t *ctlog_n, uint32_t *rlog_n,
                                                 unsigned long long *hzst) {
    const uint32_t t = threadIdx.x;
    if (t < 3) seq[t] = 0u;
    if (t == 3) seq[3] = ~0u;
    if (t < 2) ctlog_n[t] = 0u;
    if (t < 2 && rlog_n) rlog_n[t] = 0u;
    if (hzst)
        for (uint32_t k = t; k < 272; k += 256) hzst[k] = 0ull;
}
// A log of deferred CT4 writes {order, key[4], value[12], pad[3]} applied in
// order (k_ctlog_max / k_ctlog_apply: the last writer of a key wins).
// nlog: an upper bound of the entry count (*d_n, read by the kernels): no host
// round trip for the count.
// cfgs (per-endpoint CT maps): each entry into its program's own map instead of ct.
static int ctlog_apply(EgWs &ew, const uint32_t *lg, const uint32_t *d_n, uint32_t nlog, const gf_htab_desc &ct,
                       uint32_t *ct_count, hipStream_t s, const gf_lxc_dev *cfgs = nullptr) {
    if (!nlog) return 0;
    uint32_t cap = 1023;                               // the set for the bound, at <= 1/2 load
    while ((uint64_t)cap + 1 < 2ull * nlog) cap = cap * 2 + 1;
    const size_t tb = (size_t)(cap + 1) * 8;
    if (ew.ckey.bytes < tb) {                           // a new set: zero once (k_ctlog_apply keeps it zero)
        if (ew.ckey.ensure(tb)) return -ENOMEM;
        if (hip_ok(hipMemsetAsync(ew.ckey.p, 0, tb, s), "ct log set")) return -EIO;
    }
    ProfScope ps("k_ctlog_apply", s);
    const uint32_t gs = std::min<uint32_t>((cap + BLOCK) / BLOCK, 2048u);   // grid-stride over the set
    const uint32_t gl = (nlog + BLOCK - 1) / BLOCK;
    if (cfgs) {
        hipLaunchKernelGGL(k_ctlog_max<true>, dim3(gl), dim3(BLOCK), 0, s, lg, d_n, (unsigned long long *)ew.ckey.p, cap);
        hipLaunchKernelGGL(k_ctlog_apply<true>, dim3(gs), dim3(BLOCK), 0, s, lg, d_n, (unsigned long long *)ew.ckey.p, cap,
                           gf_htab_desc{}, nullptr, cfgs);
    } else {
        hipLaunchKernelGGL(k_ctlog_max<false>, dim3(gl), dim3(BLOCK), 0, s, lg, d_n, (unsigned long long *)ew.ckey.p, cap);
        hipLaunchKernelGGL(k_ctlog_apply<false>, dim3(gs), dim3(BLOCK), 0, s, lg, d_n, (unsigned long long *)ew.ckey.p,
                           cap, ct, ct_count, nullptr);
    }
    return hip_ok(hipGetLastError(), "k_ctlog_apply");
}
// One ordered run of an egress batch: check = run the ordering check first (a
// flagged batch is split into runs, each through this function again); lru = the
// LRU stand-in after it (once per classify call).
static int egress_call(const std::shared_ptr<PolicyArray> &a, const gf_lxc_batch *b, uint32_t now_sec,
                       gf_egress_out *out, uint8_t *snap_out, hipStream_t s, bool check, bool lru, uint32_t depth = 0) {
    const gf_frames &fr = b->frames;
    const uint32_t n = fr.n, S = fr.snap_stride;
    if (n == 0) return 0;
    check = check && n > 1;
    int r;
    std::vector<std::shared_ptr<ProgLxc>> progs;
    if ((r = prog_table(a, s, progs))) return r;
    CtMaps cm;
    if ((r = ct_maps_of(progs, cm))) return r;
    const bool pct = cm.pct;                           // per-endpoint CT maps (ConntrackLocal)
    std::shared_ptr<Map> ct4m = pct ? nullptr : cm.one(4), ct6m = pct ? nullptr : cm.one(6);
    uint32_t strict = 0;
    gf_htab_desc cfg_ct4{}, cfg_ct6{};
    if ((r = ct_limits(ct4m, ct6m, n, 3, s, strict, cfg_ct4, cfg_ct6))) return r;
    if (pct && (r = ct_limits_pct(cm, n, 3, s, strict))) return r;   // a family's bit: one of its maps could fill
    auto lxc = node_map(1), tun = node_map(2);
    if ((r = push_map(lxc, s)) || (r = push_map(tun, s))) return r;
    EgWs &ew = eg_ws();
    auto grow = [](DevBuf &d, size_t want) -> int { return d.bytes >= want ? 0 : d.ensure(want); };
    uint32_t hmask = 1023, amask = 1023;                 // conn keys at <= 1/2 load, up to 4 aux keys at <= 1/2
    while (check && (uint64_t)hmask + 1 < 2ull * n) hmask = hmask * 2 + 1;
    while (check && (uint64_t)amask + 1 < 8ull * n) amask = amask * 2 + 1;
    if ((r = grow(ew.erec, (size_t)n * sizeof(EgRec))) || (r = grow(ew.rec2, (size_t)n * sizeof(gf_rec))) ||
        (r = grow(ew.key2, (size_t)n * 4)) || (r = grow(ew.seq, 16)) || (r = grow(ew.ctlog_n, 8)) ||
        (r = grow(ew.ctlog, (size_t)n * GF_CTLOG_WORDS * 4)) || (r = grow(ew.s6, (size_t)n * 32)) || (r = grow(ew.hzst, 272 * 8)) || (r = ws_grow(n)))
        return r;
    if (check && ((r = grow(ew.hzk, (size_t)n * 8 * GF_HZ_NK)) || (r = grow(ew.hzfl, (size_t)n)) ||
                  (r = grow(ew.hztk, (size_t)(hmask + 1) * 8)) || (r = grow(ew.hztf, (size_t)(hmask + 1) * 16)) ||
                  (r = grow(ew.hzak, (size_t)(amask + 1) * 8)) || (r = grow(ew.hzaf, (size_t)(amask + 1) * 8))))
        return r;
    // In place (snap_out == the frames) with the check: the flagged pass must leave
    // the frames as they came, so the rewrites go to scratch and are copied at the end
    // (also when tracing: TRACE_FROM_LXC captures the frames as sent).
    PolicyPass pass;                                    // the deliveries' handle_policy pass, below
    pass.kind = PassKind::Egress;
    pass.on = event_ring().records && array_traces(a);
    pass.orig = fr.snap; pass.lxc_id = b->lxc_id;
    if (pass.on && (r = trace_prepare(n, false, s))) return r;
    const bool inplace = (check || pass.on) && snap_out == fr.snap;
    uint8_t *wsnap = inplace ? nullptr : snap_out;
    if (!wsnap) {
        if ((r = grow(ew.snap, (size_t)n * S))) return r;
        wsnap = (uint8_t *)ew.snap.p;
    }
    const gf_node_cfg &node = node_cfg();
    EgDev E{};
    E.cfgs = (const gf_lxc_dev *)a->d_cfgs.p;
    E.slot_of = (const uint16_t *)a->d_slot_of_lxc.p;
    E.K = gf_key_for(n);
    E.ct4 = cfg_ct4; E.ct6 = cfg_ct6;
    if ((r = grow(ew.v6blk, (n + BLOCK - 1) / BLOCK))) return r;
    E.v6blk = (uint8_t *)ew.v6blk.p;
    E.s6out = (uint8_t *)ew.s6.p; E.d6out = (uint8_t *)ew.s6.p + 16;   // interleaved (IngCtx::a6_stride 32)
    memcpy(E.router6, node.router_ip6, 16); memcpy(E.host6, node.host_ip6, 16);
    if (lxc) {
        E.lxc = lxc->hdesc();
        front_addr_set(lxc, s, E.lxset, E.lxbits, E.lxzero);
    }
    if (tun) {
        E.tunnel = tun->hdesc();
        front_addr_set(tun, s, E.tnset, E.tnbits, E.tnzero);
    }
    E.snap = wsnap; E.stride = S; E.now = now_sec; E.host_ifindex = host_ifindex();
    E.encap_ifindex = node.encap_ifindex;
    E.cluster_range = node.ipv4_cluster_range; E.cluster_mask = node.ipv4_cluster_mask;
    E.loopback = node.ipv4_loopback; E.ipv4_mask = node.ipv4_mask;
    memcpy(E.host_mac, node.host_mac, 6);
    E.strict = strict;
    E.seq = (uint32_t *)ew.seq.p;
    E.ctlog = (uint32_t *)ew.ctlog.p; E.ctlog_n = (uint32_t *)ew.ctlog_n.p;
    E.rec2 = (gf_rec *)ew.rec2.p; E.key2 = (uint32_t *)ew.key2.p;
    // Connection groups for IPv4 (EgDev::conn): off when CT4 inserts are counted
    // exactly (strict: the batch runs as one bucket anyway).
    static const bool no_conn = getenv("GF_EG_PAIRS") != nullptr;   // diagnosis: address-pair groups only
    const bool conn = ct4m && !(strict & 1u) && !no_conn;
    uint32_t *d_rn = nullptr;                          // [0] related entries logged, [1] pair-group fallback
    if (conn) {
        // the related entries' set (RelSet): 4n slots keep it at most half full (<= 2n
        // writes, one per new connection in each pass); batches too large for 32-bit slot
        // numbers keep the write log
        uint64_t ns = 1024;
        while (ns < 4ull * n) ns *= 2;
        const bool rset = ns <= (1ull << 31);
        if ((r = grow(ew.keysP, (size_t)n * 4)) || (r = grow(ew.key2P, (size_t)n * 4)) || (r = grow(ew.rlog_n, 8)) ||
            (!rset && (r = grow(ew.rlog, (size_t)2 * n * GF_CTLOG_WORDS * 4))))
            return r;
        d_rn = (uint32_t *)ew.rlog_n.p;
        E.conn = 1; E.cflag = d_rn + 1;
        E.keysP = (uint32_t *)ew.keysP.p; E.key2P = (uint32_t *)ew.key2P.p;
        E.rlog = (uint32_t *)ew.rlog.p; E.rlog_n = d_rn;
        if (rset) {
            // zeroed when allocated, and left zero by k_rset_apply, which clears every
            // slot a run claimed
            const size_t sb = (size_t)(ns + 1) * 16;
            if (ew.rsslot.bytes < sb) {
                if (ew.rsslot.ensure(sb)) return -ENOMEM;
                if (hip_ok(hipMemsetAsync(ew.rsslot.p, 0, sb, s), "related set")) return -EIO;
            }
            if ((r = grow(ew.rslist, (size_t)2 * n * 4 + 4))) return r;
            E.rs.slot = (unsigned long long *)ew.rsslot.p;
            E.rs.list = (uint32_t *)ew.rslist.p; E.rs.list_n = d_rn; E.rs.mask = (uint32_t)(ns - 1);
            E.rlog = E.rs.list;                          // (marks the set in use for the deliveries' pass)
        }
    }
    uint32_t *d_hz = (uint32_t *)ew.seq.p + 1;           // word 1 of the seq buffer: the hazard flag
    if (check) {
        E.hz_k = (uint64_t *)ew.hzk.p; E.hz_fl = (uint8_t *)ew.hzfl.p; E.hz = d_hz;
        if ((r = vip_sets(progs, ew, s))) return r;
        if (ew.vip4_any) { E.vip4 = (const uint32_t *)ew.vip4.p; E.vip4_mask = ew.vip4_mask; }
        if (ew.vip6_any) { E.vip6 = (const uint4 *)ew.vip6.p; E.vip6_mask = ew.vip6_mask; }
    }
    E.X.snap = nullptr; E.X.snap_stride = S; E.X.now = now_sec; E.X.gw = node.ipv4_gateway;   // writes: k_eg_groups
    memcpy(E.X.host6, node.host_ip6, 16);
    if (pass.on) { E.X.tmark = (uint8_t *)trace_ws().mark.p; E.X.tcap = (uint8_t *)trace_ws().px.p; }
    if ((r = px_log_begin(n, s, E.X))) return r;
    unsigned long long *sink = (unsigned long long *)stats_sink();
    // With the check, the front counts into a scratch block folded into the sink
    // only when the batch runs as it is (a flagged batch's runs count themselves).
    unsigned long long *fsink = sink;
    if (check && sink) fsink = (unsigned long long *)ew.hzst.p;
    hipLaunchKernelGGL(k_eg_init, dim3(1), dim3(256), 0, s, (uint32_t *)ew.seq.p, (uint32_t *)ew.ctlog_n.p, d_rn,
                       fsink != sink ? fsink : nullptr);
    Workspace &w = ws();
    {
        ProfScope ps("k_eg_front", s);
        // the IPv4 kernel's LDS rows: one per lane, the staged header bytes (<= GF_EG_STAGE)
        const uint32_t eg_lds = BLOCK * std::min<uint32_t>(S, GF_EG_STAGE);
        hipLaunchKernelGGL(k_eg_front<4>, dim3((n + BLOCK - 1) / BLOCK), dim3(BLOCK), eg_lds, s, fr, b->lxc_id, b->flow_hash,
                           E, (EgRec *)ew.erec.p, (uint32_t *)w.keys.p, out, fsink);
        hipLaunchKernelGGL(k_eg_front<6>, dim3((n + BLOCK - 1) / BLOCK), dim3(BLOCK), 16, s, fr, b->lxc_id, b->flow_hash,
                           E, (EgRec *)ew.erec.p, (uint32_t *)w.keys.p, out, fsink);
        hipLaunchKernelGGL(k_eg_seq_keys, dim3(grid_for(n)), dim3(BLOCK), 0, s, (const uint32_t *)ew.seq.p,
                           (const uint32_t *)E.cflag, (const uint32_t *)E.keysP, n, (uint32_t *)w.keys.p, E.K);
        if ((r = hip_ok(hipGetLastError(), "k_eg_front"))) return r;
    }
    if (check) {
        ProfScope ps("k_hz_check", s);
        if (ew.hz_cap != hmask + 1 || ew.hz_gen >= 0xffffu) {   // new table or wrapped generation
            if (hip_ok(hipMemsetAsync(ew.hztk.p, 0, (size_t)(hmask + 1) * 8, s), "hz keys") ||
                hip_ok(hipMemsetAsync(ew.hztf.p, 0, (size_t)(hmask + 1) * 16, s), "hz first"))
                return -EIO;
            ew.hz_cap = hmask + 1; ew.hz_gen = 0;
        }
        const HzGen C{(unsigned long long *)ew.hztk.p, (unsigned long long *)ew.hztf.p, hmask, ++ew.hz_gen};
        const HzTab A{(unsigned long long *)ew.hzak.p, (uint32_t *)ew.hzaf.p, amask};
        hipLaunchKernelGGL(k_hz_clear, dim3(std::min<uint32_t>((amask + 1) / BLOCK, 8192)), dim3(BLOCK), 0, s, A,
                           (const uint32_t *)d_hz);
        hipLaunchKernelGGL(k_hz_insert, dim3(grid_for(n)), dim3(BLOCK), 0, s, (const uint64_t *)ew.hzk.p,
                           (const uint8_t *)ew.hzfl.p, n, (const uint32_t *)d_hz, C, A);
        hipLaunchKernelGGL(k_hz_probe, dim3(grid_for(n)), dim3(BLOCK), 0, s, (const uint64_t *)ew.hzk.p,
                           (const uint8_t *)ew.hzfl.p, n, C, A, strict, d_hz);
        if ((r = hip_ok(hipGetLastError(), "k_hz_check"))) return r;
        // the check's verdict goes to pinned host memory behind an event: the host
        // reads it while the device already builds the schedule (no stream sync)
        if (!ew.h_hz && (hip_ok(hipHostMalloc((void **)&ew.h_hz, 16, hipHostMallocDefault), "hz host") ||
                         hip_ok(hipEventCreateWithFlags(&ew.ev_hz, hipEventDisableTiming), "hz event")))
            return -EIO;
        if (hip_ok(hipMemcpyAsync(ew.h_hz, d_hz, 12, hipMemcpyDeviceToHost, s), "hz flag") ||
            hip_ok(hipEventRecord(ew.ev_hz, s), "hz record"))
            return -EIO;
    }
    if ((r = schedule_groups(n, s, true))) return r;   // (reads only the front's keys: harmless on a flagged batch)
    host_mark("front+sched");
    // k_eg_groups is queued before the host looks at the ordering check: it reads the
    // check's flag itself and idles on a flagged batch (no map state changes then), so
    // the device has the schedule and the groups to run while the host waits for the
    // check's verdict and enqueues the rest of the call behind them
    {
        const uint32_t grid = std::min(resident_blocks(8), (n + BLOCK - 1) / BLOCK);
        ProfScope ps("k_eg_groups", s);
        // one launch per family: IPv4 stages one header row per lane in LDS (eg_row_bytes of the snap
        // stride), IPv6 none; the count word is the family's CT map's, null with per-endpoint maps
        // (pct: each packet's change goes to its own program's map)
        auto launch = [&](auto k4, auto k6) {
            auto go = [&](auto kern, size_t lds, const std::shared_ptr<Map> &ct) {
                hipLaunchKernelGGL(kern, dim3(grid), dim3(BLOCK), lds, s, E, (uint32_t *)w.sched.p, (const uint2 *)w.order.p,
                                   (const uint32_t *)w.perm.p, (const EgRec *)ew.erec.p, out, (gf_rec *)ew.rec2.p,
                                   (uint32_t *)ew.key2.p, ct ? (uint32_t *)ct->d_count.p : nullptr, sink);
            };
            go(k4, BLOCK * eg_row_bytes(S), ct4m);
            go(k6, 16, ct6m);
        };
        if (pct) launch(k_eg_groups<4, true>, k_eg_groups<6, true>);
        else launch(k_eg_groups<4>, k_eg_groups<6>);
        if ((r = hip_ok(hipGetLastError(), "k_eg_groups"))) return r;
    }
    uint32_t hz = 0, hz_first = 0;
    if (check) {
        if (hip_ok(hipEventSynchronize(ew.ev_hz), "hz sync")) return -EIO;
        host_mark("hzwait");
        hz = ew.h_hz[0]; hz_first = ew.h_hz[2];
    }
    if (hz & 2u) {
        if (getenv("GF_HZ_DEBUG")) fprintf(stderr, "[gf] egress n=%u: a CT map could fill, one packet at a time\n", n);
        return egress_each(a, b, now_sec, out, snap_out, s, lru);
    }
    if (hz) return egress_ordered(a, b, now_sec, out, snap_out, s, lru, hz_first, depth);
    // ct_create4's deferred service entries, in batch order; every count from here
    // on is read on the device (no host round trip inside the call)
    if (check && sink) {
        hipLaunchKernelGGL(k_stats_fold, dim3(1), dim3(256), 0, s, (const unsigned long long *)fsink, sink);
        if ((r = hip_ok(hipGetLastError(), "k_stats_fold"))) return r;
    }
    if (ct4m && (r = ctlog_apply(ew, (const uint32_t *)ew.ctlog.p, (const uint32_t *)ew.ctlog_n.p, n, cfg_ct4,
                                 (uint32_t *)ct4m->d_count.p, s)))
        return r;
    if (pct && !cm.m4.empty() &&
        (r = ctlog_apply(ew, (const uint32_t *)ew.ctlog.p, (const uint32_t *)ew.ctlog_n.p, n, gf_htab_desc{}, nullptr, s,
                         (const gf_lxc_dev *)a->d_cfgs.p)))
        return r;
    for (auto *v : {&cm.m4, &cm.m6})
        for (auto &m : *v) m->device_modified();
    // The egress redirects' cilium_proxy{4,6} updates stay in the log: the
    // deliveries' handle_policy appends theirs and the whole log is applied in
    // packet order after it (nothing on these paths reads the proxy maps).
    // handle_policy of the local deliveries (the tail calls of ipv4_local_delivery)
    gf_pkt_cols c2{};
    c2.n = n;
    c2.len = fr.len;
    c2.flow_hash = b->flow_hash;
    c2.saddr6 = (const uint8_t *)ew.s6.p; c2.daddr6 = (const uint8_t *)ew.s6.p + 16;   // IPv6 deliveries (if any)
    // the deliveries' keys: their connections, or address pairs when the run fell back
    // k_eg_groups wrote them in batch order: they become the workspace's records and
    // keys by exchanging the buffers (the workspace's old ones are the next call's
    // pass-2 buffers), not by copying n records; a fallen-back run takes the pair
    // keys on the device (k_eg_seq_keys' rule, *cflag)
    pass.pack = [&](const uint16_t *, gf_rec *, uint32_t *) -> int {
        Workspace &w = ws();
        std::swap(w.rec.p, ew.rec2.p); std::swap(w.rec.bytes, ew.rec2.bytes);
        std::swap(w.keys.p, ew.key2.p); std::swap(w.keys.bytes, ew.key2.bytes);
        if (conn) {
            hipLaunchKernelGGL(k_eg_pick_keys, dim3(grid_for(n)), dim3(BLOCK), 0, s, (const uint32_t *)E.cflag,
                               (const uint32_t *)ew.key2P.p, n, (uint32_t *)w.keys.p);
            return hip_ok(hipGetLastError(), "k_eg_pick_keys");
        }
        return 0;
    };
    if (conn) { pass.rlog = E.rlog; pass.rlog_n = d_rn; pass.rlog_off = E.cflag; pass.rs = E.rs; }
    pass.pout = (uint8_t *)out;
    pass.ev_len = fr.len;
    pass.ev_snap = wsnap;
    pass.ev_stride = S;
    pass.wsnap = wsnap;
    pass.lru = lru && !conn;                            // (with connection groups: after the related entries, below)
    pass.px_keep = true;                                // the from-container pass' redirects are in the log
    if ((r = ingress_run(a, &c2, now_sec, s, pass))) return r;
    if (conn && E.rs.slot) {                           // both passes' related entries: each key's last writer
        ProfScope ps("k_ctlog_apply", s);
        // the deliveries' records are the workspace's now (the pack swap above)
        hipLaunchKernelGGL(k_rset_apply, dim3(std::min<uint32_t>(grid_for(2 * n), 2048u)), dim3(BLOCK), 0, s, E.rs,
                           (const EgRec *)ew.erec.p, (const gf_rec *)ws().rec.p, E.cfgs, cfg_ct4,
                           (uint32_t *)ct4m->d_count.p, now_sec);
        if ((r = hip_ok(hipGetLastError(), "k_rset_apply"))) return r;
    } else if (conn) {                                 // both passes' related entries, in packet order
        if ((r = ctlog_apply(ew, (const uint32_t *)ew.rlog.p, d_rn, 2 * n, cfg_ct4, (uint32_t *)ct4m->d_count.p, s)))
            return r;
    }
    if (conn) {
        ct4m->device_modified();
        if (lru && ((r = lru_evict(ct4m, now_sec, s)) || (r = lru_evict(ct6m, now_sec, s)))) return r;
    }
    static const bool logstats = getenv("GF_EG_LOGSTATS") != nullptr;   // diagnostics: syncs the stream
    if (logstats) {
        uint32_t c[2] = {0, 0}, rc[2] = {0, 0};
        if (!hip_ok(hipStreamSynchronize(s), "logstats") &&
            !hip_ok(hipMemcpy(c, ew.ctlog_n.p, 8, hipMemcpyDeviceToHost), "logstats") &&
            (!conn || !hip_ok(hipMemcpy(rc, d_rn, 8, hipMemcpyDeviceToHost), "logstats")))
            fprintf(stderr, "[gf] egress n=%u: service-entry log %u, related-entry log %u (fallback %u)\n", n, c[0], rc[0],
                    rc[1]);
    }
    if (inplace && hip_ok(hipMemcpyAsync(snap_out, wsnap, (size_t)n * S, hipMemcpyDeviceToDevice, s), "snap copy"))
        return -EIO;
    return 0;
}

// A flagged batch: the cut points (a new run starts at a packet whose reverse
// direction is in the current run, and around every single-bucket tuple), then
// every run through egress_call in order.  Nothing of the flagged pass changed
// the maps: k_eg_groups idled, and the front only reads them.
static int egress_greedy(const std::shared_ptr<PolicyArray> &a, const gf_lxc_batch *b, uint32_t now_sec,
                         gf_egress_out *out, uint8_t *snap_out, hipStream_t s, bool lru);
static int egress_ordered(const std::shared_ptr<PolicyArray> &a, const gf_lxc_batch *b, uint32_t now_sec,
                          gf_egress_out *out, uint8_t *snap_out, hipStream_t s, bool lru, uint32_t first, uint32_t depth) {
    const uint32_t n = b->frames.n;
    if (getenv("GF_HZ_DEBUG")) fprintf(stderr, "[gf] egress n=%u: ordering hazard at %u (run %u)\n", n, first, depth + 1);
    if (first == 0 || first >= n || depth >= 32) return egress_greedy(a, b, now_sec, out, snap_out, s, lru);
    // [0, first) has no hazard; the rest runs after it, checked again
    std::vector<uint32_t> cut{0, first};
    int r = egress_runs(a, b, now_sec, out, snap_out, s, false, cut);
    if (r) return r;
    const uint32_t S = b->frames.snap_stride;
    gf_lxc_batch rest = *b;
    rest.frames.n = n - first;
    rest.frames.snap = b->frames.snap + (size_t)first * S;
    rest.frames.len = b->frames.len + first;
    if (b->lxc_id) rest.lxc_id = b->lxc_id + first;
    if (b->flow_hash) rest.flow_hash = b->flow_hash + first;
    return egress_call(a, &rest, now_sec, out + first, snap_out ? snap_out + (size_t)first * S : nullptr, s, true, lru,
                       depth + 1);
}
// Many runs: the cut points on the host, in one pass over the batch's keys.
static int egress_greedy(const std::shared_ptr<PolicyArray> &a, const gf_lxc_batch *b, uint32_t now_sec,
                         gf_egress_out *out, uint8_t *snap_out, hipStream_t s, bool lru) {
    EgWs &ew = eg_ws();
    const uint32_t n = b->frames.n;
    std::vector<uint64_t> K((size_t)n * GF_HZ_NK);
    std::vector<uint8_t> fl(n);
    if (hip_ok(hipMemcpyAsync(K.data(), ew.hzk.p, K.size() * 8, hipMemcpyDeviceToHost, s), "hz keys") ||
        hip_ok(hipMemcpyAsync(fl.data(), ew.hzfl.p, n, hipMemcpyDeviceToHost, s), "hz fl") ||
        hip_ok(hipStreamSynchronize(s), "hz sync"))
        return -EIO;
    // the rules of k_hz_insert / k_hz_probe over the current run (keys are odd:
    // bit 0 carries a connection key's direction)
    std::vector<uint32_t> cut{0};
    std::unordered_set<uint64_t> seen;
    const uint64_t D = 1ull;
    uint32_t why[5] = {0, 0, 0, 0, 0};
    auto k = [&](uint32_t which, uint32_t j) { return K[(size_t)which * n + j] & ~D; };
    for (uint32_t j = 0; j < n; j++) {
        const uint32_t f = fl[j];
        if (!(f & GF_HZ_VALID)) continue;
        const bool h0 = seen.count(k(1, j) | ((f & GF_HZ_DIRE) ? 0ull : D)) != 0;
        const bool h1 = (f & GF_HZ_ICMP) && seen.count(k(3, j) ^ 2ull) != 0;
        const bool h2 = seen.count((k(3, j) ^ GF_HZ_ICMPSALT) & ~D) != 0;
        const bool h3 = (f & GF_HZ_LOOP) && (seen.count(k(0, j)) || seen.count(k(0, j) | D));
        const bool h4 = (f & GF_HZ_VIP) && seen.count(k(4, j) ^ 2ull) != 0;
        why[0] += h0; why[1] += h1; why[2] += h2; why[3] += h3; why[4] += h4;
        if (h0 || h1 || h2 || h3 || h4) { cut.push_back(j); seen.clear(); }
        if (f & GF_HZ_DLV) seen.insert(k(0, j) | ((f & GF_HZ_DIRI) ? D : 0ull));
        seen.insert(k(2, j) ^ 2ull);
        if (f & GF_HZ_ICMP) seen.insert((k(2, j) ^ GF_HZ_ICMPSALT) & ~D);
        seen.insert(k(4, j) ^ 2ull);
        seen.insert(k(5, j) ^ 2ull);
    }
    if (cut.back() != n) cut.push_back(n);
    if (getenv("GF_HZ_DEBUG"))
        fprintf(stderr, "[gf] egress n=%u: %zu ordered runs (reply %u, icmp-after %u, after-icmp %u, loopback %u, vip %u)\n",
                n, cut.size() - 1, why[0], why[1], why[2], why[3], why[4]);
    return egress_runs(a, b, now_sec, out, snap_out, s, lru, cut);
}

// The runs [cut[k], cut[k+1]) of a batch through egress_call, in order; the LRU
// stand-in after the last.
static int egress_runs(const std::shared_ptr<PolicyArray> &a, const gf_lxc_batch *b, uint32_t now_sec,
                       gf_egress_out *out, uint8_t *snap_out, hipStream_t s, bool lru, const std::vector<uint32_t> &cut) {
    const uint32_t S = b->frames.snap_stride;
    for (size_t k = 0; k + 1 < cut.size(); k++) {
        const uint32_t lo = cut[k], hi = cut[k + 1];
        gf_lxc_batch sub = *b;
        sub.frames.n = hi - lo;
        sub.frames.snap = b->frames.snap + (size_t)lo * S;
        sub.frames.len = b->frames.len + lo;
        if (b->lxc_id) sub.lxc_id = b->lxc_id + lo;
        if (b->flow_hash) sub.flow_hash = b->flow_hash + lo;
        int r = egress_call(a, &sub, now_sec, out + lo, snap_out ? snap_out + (size_t)lo * S : nullptr, s, false,
                            lru && k + 2 == cut.size());
        if (r) return r;
    }
    return 0;
}

extern "C" int gf_lxc_egress_classify(int array, const gf_lxc_batch *b, uint32_t now_sec, gf_egress_out *out,
                                      uint8_t *snap_out, void *stream) {
    std::shared_lock<std::shared_mutex> g(prog_lock());
    auto a = get_as<PolicyArray>(array);
    if (!a) return -EBADF;
    if (!b) return -EFAULT;
    const gf_frames &fr = b->frames;
    if (fr.n == 0) return 0;
    if (!fr.snap || !fr.len || !out) return -EFAULT;
    if (fr.snap_stride < 34) return -EINVAL;           // an Ethernet + IPv4 header at least
    if (fr.n > (1u << 30)) return -E2BIG;
    // the from-container program without conntrack (bpf_lxc.c:429-674 over the stub ct_*) is not built
    if (array_noct(a)) return -EOPNOTSUPP;
    hipStream_t s = (hipStream_t)stream;
    HostMarks hm;
    CtxScope cx(s);
    std::lock_guard<std::mutex> ag(a->mu);
    MapLocks L;
    lock_array_maps(L, a);
    L.lock();
    CallOrder co(s, L, a.get());
    host_mark("locks");
    static const bool nocheck = getenv("GF_EG_NOCHECK") != nullptr;     // diagnosis only: the unordered schedule
    static const bool dbg = getenv("GF_HZ_DEBUG") != nullptr;
    if (!dbg) return egress_call(a, b, now_sec, out, snap_out, s, !nocheck, true);
    (void)hipStreamSynchronize(s);
    auto t0 = std::chrono::steady_clock::now();
    int r = egress_call(a, b, now_sec, out, snap_out, s, !nocheck, true);
    (void)hipStreamSynchronize(s);
    fprintf(stderr, "[gf] egress n=%u: %.3f ms\n", fr.n,
            std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    return r;
}
