// gf_host_programs.h — the first block of the C ABI: gf_parse_frames; gf_xdp_prog_load /
// gf_xdp_classify; gf_lb_prog_load / gf_lb_classify; gf_lxc_prog_load; gf_set_event_ring;
// gf_prof_*; gf_policy_array_create / _update (included by gf_kernels.hip after gf_host_ctx.h:
// its contexts, check_cols and CallOrder; it launches k_parse, k_xdp, k_xdp_lds and k_lb).

extern "C" {

int gf_parse_frames(const gf_frames *fr, gf_pkt_cols_out *o, void *stream) {
    if (!fr || !o) return -EFAULT;
    if (fr->n == 0) return 0;
    if (!fr->snap || !fr->len || !o->ethertype || !o->saddr4 || !o->daddr4 || !o->proto || !o->l4_off ||
        !o->l4w0 || !o->l4w3)
        return -EFAULT;
    if (fr->snap_stride < 14) return -EINVAL;
    ProfScope ps("k_parse", (hipStream_t)stream);
    hipLaunchKernelGGL(k_parse, dim3(grid_for(fr->n)), dim3(BLOCK), 0, (hipStream_t)stream, *fr, *o);
    return hip_ok(hipGetLastError(), "k_parse");
}

int gf_xdp_prog_load(const gf_xdp_cfg *cfg) {
    std::unique_lock<std::shared_mutex> g(prog_lock());
    if (!cfg) return -EFAULT;
    auto p = std::make_shared<ProgXdp>();
    p->cfg = *cfg;
    auto bind = [](int h, uint32_t ksz, bool lpm, std::shared_ptr<Map> &out) -> int {
        if (!h) return 0;
        auto m = get_map(h);
        if (!m) return -EBADF;
        if (m->ksz != ksz || m->is_lpm() != lpm) return -EINVAL;
        out = m;
        return 0;
    };
    int r;
    if ((r = bind(cfg->cidr4_hmap, 8, false, p->m4h))) return r;
    if ((r = bind(cfg->cidr4_lmap, 8, true, p->m4l))) return r;
    if ((r = bind(cfg->cidr6_hmap, 20, false, p->m6h))) return r;
    if ((r = bind(cfg->cidr6_lmap, 20, true, p->m6l))) return r;
    if ((r = bind(cfg->lxc_map, 20, false, p->lxc))) return r;
    if (!p->lxc) return -EINVAL;
    return new_handle(p);
}

int gf_xdp_classify(int prog, const gf_pkt_cols *pkts, uint8_t *verdict, void *stream) {
    std::shared_lock<std::shared_mutex> g(prog_lock());
    auto p = get_as<ProgXdp>(prog);
    if (!p) return -EBADF;
    int c = check_cols(pkts);
    if (c <= 0) return c;
    if (!verdict) return -EFAULT;
    hipStream_t s = (hipStream_t)stream;
    CtxScope cx(s);
    MapLocks L;
    lock_xdp_maps(L, *p);
    L.lock();
    CallOrder co(s, L);
    int r;
    if ((r = push_map(p->m4h, s)) || (r = push_map(p->m4l, s)) || (r = push_map(p->m6h, s)) ||
        (r = push_map(p->m6l, s)) || (r = push_map(p->lxc, s)))
        return r;
    XdpDev x{};
    xdp_sets(p->m4h, p->lxc, x, s);
    if (p->m4h) { x.h4 = p->m4h->hdesc(); x.has_h4 = 1; }
    if (p->m6h) { x.h6 = p->m6h->hdesc(); x.has_h6 = 1; }
    if (p->m4l) x.l4 = p->m4l->tdesc();
    if (p->m6l) x.l6 = p->m6l->tdesc();
    xdp_dir(p->m4l, x, s);
    x.lxc = p->lxc->hdesc();
    ProfScope ps("k_xdp", s);
    // The LDS variant when the LPM map has a 16-bit root (its summary is 16 KB);
    // the /32 hash and the endpoint keys join it while they fit.
    static const bool no_lds = getenv("GF_XDP_NOLDS") != nullptr;     // diagnosis: the HBM-only kernel
    if (!no_lds && x.l4.rsum && x.has_h4 && x.l4.addr_bytes == 4) {
        static const uint32_t cap = getenv("GF_XDP_LDS_KB") ? 1024u * (uint32_t)atoi(getenv("GF_XDP_LDS_KB")) : 48u * 1024u;
        XdpLds L{};
        // the /32 hash and the endpoint keys as compact address sets (4 B a slot), else
        // their slot arrays when those fit the budget
        L.h4set = x.h4set; L.h4bits = x.h4bits; L.h4zero = x.h4zero;
        L.lxset = x.lxset; L.lxbits = x.lxbits; L.lxzero = x.lxzero;
        const uint64_t hb = (uint64_t)(x.h4.mask + 1) * x.h4.slot_size, lb = (uint64_t)(x.lxc.mask + 1) * x.lxc.slot_size;
        if (!L.h4set && x.h4.slots && x.h4.ksz == 8 && hb % 16 == 0 && GF_TRIE_RSUM_BYTES + hb <= std::min(cap, 96u * 1024u))
            L.h4_bytes = (uint32_t)hb;
        const uint32_t h4b = L.h4set ? 4u << L.h4bits : L.h4_bytes;
        if (!L.lxset && x.lxc.slots && x.lxc.ksz == 20 && lb % 16 == 0 && GF_TRIE_RSUM_BYTES + h4b + lb <= cap)
            L.lxc_bytes = (uint32_t)lb;
        const uint32_t lds = GF_TRIE_RSUM_BYTES + h4b + (L.lxset ? 4u << L.lxbits : L.lxc_bytes);
        // the address sets count against the budget too: larger maps take k_xdp,
        // which reads the same sets and the root summary through L2
        static std::atomic<uint32_t> lds_set{0};
        bool fits = lds <= std::max(cap, GF_TRIE_RSUM_BYTES);
        if (fits && lds > lds_set.load()) {
            fits = hipFuncSetAttribute((const void *)k_xdp_lds, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) ==
                   hipSuccess;
            if (fits) {
                uint32_t cur = lds_set.load();
                while (lds > cur && !lds_set.compare_exchange_weak(cur, lds)) {}
            } else {
                (void)hipGetLastError();
            }
        }
        if (fits) {
        const uint32_t per_cu = lds <= 78u * 1024u ? 2u : 1u;
        static const uint32_t grid_env = getenv("GF_XDP_GRID") ? (uint32_t)atoi(getenv("GF_XDP_GRID")) : 0u;   // diagnosis
        const uint32_t grid = grid_env ? grid_env
                                       : std::max<uint32_t>(1u, std::min<uint32_t>(resident_blocks(per_cu), (pkts->n + 1023) / 1024));
        hipLaunchKernelGGL(k_xdp_lds, dim3(grid), dim3(1024), lds, s, *pkts, x, L, verdict,
                           (unsigned long long *)stats_sink());
        return hip_ok(hipGetLastError(), "k_xdp_lds");
        }
    }
    hipLaunchKernelGGL(k_xdp, dim3(stream_grid(pkts->n)), dim3(BLOCK), 0, s, *pkts, x, verdict,
                       (unsigned long long *)stats_sink());
    return hip_ok(hipGetLastError(), "k_xdp");
}

int gf_lb_prog_load(const gf_lb_cfg *cfg) {
    std::unique_lock<std::shared_mutex> g(prog_lock());
    if (!cfg) return -EFAULT;
    auto p = std::make_shared<ProgLb>();
    p->cfg = *cfg;
    if (cfg->lb4_services) {
        p->lb4 = get_map(cfg->lb4_services);
        if (!p->lb4) return -EBADF;
        if (p->lb4->ksz != 8 || p->lb4->vsz != 12 || p->lb4->is_lpm()) return -EINVAL;
    }
    if (cfg->lb6_services) {
        p->lb6 = get_map(cfg->lb6_services);
        if (!p->lb6) return -EBADF;
        if (p->lb6->ksz != 20 || p->lb6->vsz != 24 || p->lb6->is_lpm()) return -EINVAL;
    }
    return new_handle(p);
}

int gf_lb_classify(int prog, const gf_pkt_cols *pkts, gf_lb_out *out, uint8_t *nd6, void *stream) {
    std::shared_lock<std::shared_mutex> g(prog_lock());
    auto p = get_as<ProgLb>(prog);
    if (!p) return -EBADF;
    int c = check_cols(pkts);
    if (c <= 0) return c;
    if (!out) return -EFAULT;
    hipStream_t s = (hipStream_t)stream;
    CtxScope cx(s);
    MapLocks ML;
    ML.add(p->lb4); ML.add(p->lb6);
    ML.lock();
    CallOrder co(s, ML);
    int r;
    if ((r = push_map(p->lb4, s)) || (r = push_map(p->lb6, s))) return r;
    const LbDev L = lb_dev(*p);
    ProfScope ps("k_lb", s);
    hipLaunchKernelGGL(k_lb, dim3(stream_grid(pkts->n)), dim3(BLOCK), 0, s, *pkts, L, out, nd6,
                       (unsigned long long *)stats_sink());
    return hip_ok(hipGetLastError(), "k_lb");
}

int gf_lxc_prog_load(const gf_lxc_cfg *cfg) {
    std::unique_lock<std::shared_mutex> g(prog_lock());
    if (!cfg) return -EFAULT;
    if (cfg->n_l4_ingress > GF_MAX_L4_INGRESS || cfg->n_l4_egress > GF_MAX_L4_INGRESS ||
        cfg->n_portmap > GF_MAX_PORTMAP)
        return -E2BIG;
    // CONNTRACK undefined: CFG_L3L4_* is refused (bpf/lib/l4.h:138-139); the CT maps and
    // CONNTRACK_ACCOUNTING mean nothing to the stub ct_* (conntrack.h:582-617)
    const bool noct = (cfg->flags & GF_LXC_F_NO_CONNTRACK) != 0;
    if (noct && (cfg->n_l4_ingress || cfg->n_l4_egress)) return -EINVAL;
    if (noct && (cfg->flags & GF_LXC_F_DEBUG)) return -EOPNOTSUPP;   // (the CT-off kernel sends no debug messages)
    // GF_LXC_F_LB_DEBUG needs no rule: without DEBUG cilium_dbg_lb is the empty cilium_dbg (dbg.h:134-233)
    auto p = std::make_shared<ProgLxc>();
    p->cfg = *cfg;
    if (noct) { p->cfg.ct_map4 = p->cfg.ct_map6 = 0; p->cfg.flags &= ~GF_LXC_F_CT_ACCOUNTING; }
    struct B { int h; uint32_t k, v; bool lpm; std::shared_ptr<Map> *out; };
    B binds[] = {
        {cfg->policy_map, 8, 24, false, &p->policy}, {p->cfg.ct_map4, 14, 48, false, &p->ct4},
        {p->cfg.ct_map6, 40, 48, false, &p->ct6},      {cfg->cidr4_ingress_map, 8, 0, true, &p->cidr4},
        {cfg->cidr6_ingress_map, 20, 0, true, &p->cidr6}, {cfg->revnat4_map, 2, 6, false, &p->revnat4},
        {cfg->revnat6_map, 2, 18, false, &p->revnat6},
        {cfg->lb4_services, 8, 12, false, &p->lb4},      {cfg->ipcache_map, 20, 8, false, &p->ipcache},
        {cfg->cidr4_egress_map, 8, 0, true, &p->cidr4e}, {cfg->lb6_services, 20, 24, false, &p->lb6},
        {cfg->cidr6_egress_map, 20, 0, true, &p->cidr6e},
    };
    for (auto &b : binds) {
        if (!b.h) continue;
        auto m = get_map(b.h);
        if (!m) return -EBADF;
        if (m->ksz != b.k || m->is_lpm() != b.lpm || (!b.lpm && m->vsz != b.v)) return -EINVAL;
        *b.out = m;
    }
    MapLocks L;
    lock_lxc_maps(L, p);
    L.lock();
    if (p->ct4) { p->ct4->set_hash_mode(GF_HASH_CT); p->ct4->set_value_codec(GF_VCODEC_CT); p->ct4->make_fixed_capacity(gf_ct_slot_factor(p->ct4->ksz)); }
    if (p->ct6) { p->ct6->set_hash_mode(GF_HASH_CT); p->ct6->set_value_codec(GF_VCODEC_CT); p->ct6->make_fixed_capacity(gf_ct_slot_factor(p->ct6->ksz)); }
    if (p->policy) { p->policy->set_hash_mode(GF_HASH_POLICY); p->policy->set_value_codec(GF_VCODEC_POL); }
    return new_handle(p);
}

int gf_set_event_ring(const gf_event_ring *ring) {
    std::unique_lock<std::shared_mutex> g(prog_lock());
    if (!ring) { event_ring() = gf_event_ring{}; return 0; }
    if (!ring->records || !ring->count) return -EFAULT;
    event_ring() = *ring;
    return 0;
}

int gf_prof_enable(int on) {
    std::unique_lock<std::shared_mutex> g(prog_lock());
    prof_drain();
    prof().acc.clear();
    prof().on = on != 0;
    return 0;
}

int gf_prof_read(gf_prof_rec *out, int max) {
    std::unique_lock<std::shared_mutex> g(prog_lock());
    if (max < 0 || (max > 0 && !out)) return -EFAULT;
    prof_drain();
    int k = 0;
    for (auto &kv : prof().acc) {
        if (k >= max) break;
        memset(&out[k], 0, sizeof out[k]);
        strncpy(out[k].name, kv.first.c_str(), sizeof(out[k].name) - 1);
        out[k].count = kv.second.first;
        out[k].total_ms = kv.second.second;
        k++;
    }
    return k;
}

int gf_policy_array_create(void) {
    std::unique_lock<std::shared_mutex> g(prog_lock());
    return new_handle(std::make_shared<PolicyArray>());
}

int gf_policy_array_update(int array, uint32_t lxc_id, int prog) {
    std::unique_lock<std::shared_mutex> g(prog_lock());
    auto a = get_as<PolicyArray>(array);
    if (!a) return -EBADF;
    if (lxc_id > 0xffff) return -E2BIG;
    if (prog) {
        auto po = get_as<ProgLxc>(prog);
        if (!po) return -EINVAL;
        a->slots[lxc_id] = po;
    } else {
        a->slots.erase(lxc_id);
    }
    a->dirty = true;
    a->gen++;
    size_t off = 0;                                     // programs without conntrack: none, some, every one
    for (auto &kv : a->slots)
        if (kv.second->cfg.flags & GF_LXC_F_NO_CONNTRACK) off++;
    a->noct = !off ? 0 : off == a->slots.size() ? 2 : 1;
    a->dbg = false;                                     // any program with DEBUG
    for (auto &kv : a->slots)
        if (kv.second->cfg.flags & GF_LXC_F_DEBUG) a->dbg = true;
    return 0;
}

}  // extern "C"
