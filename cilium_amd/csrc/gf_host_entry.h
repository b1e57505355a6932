// gf_host_entry.h — the second block of the C ABI, every entry point that ends in ingress_run or
// sweeps a map (included by gf_kernels.hip after the host code of the handle_policy pass, whose
// PolicyPass, ingress_run, FrontLaunch and CT sweeps it calls, over gf_host_ctx.h's contexts):
// gf_policy_ingress_classify(_batches); gf_pipeline_load / _classify(_tunnel);
// gf_lb_prog_set_dstmac / gf_lb_classify_frames; gf_overlay_load / _classify(_opts);
// gf_lxc_egress_tunnel_meta; gf_host_load / _classify; gf_pipeline_partition; gf_ct_gc(_maps);
// gf_proxy_gc / gf_proxy_cleanup_port; gf_diag_wrstats; gf_ct_evict_log.

extern "C" {

int gf_policy_ingress_classify_batches(int array, uint32_t nb, const gf_pkt_cols *const *batches,
                                       const uint32_t *now_sec, gf_ingress_out *const *outs, void *stream) {
    std::shared_lock<std::shared_mutex> g(prog_lock());
    auto a = get_as<PolicyArray>(array);
    if (!a) return -EBADF;
    if (nb && (!batches || !now_sec || !outs)) return -EFAULT;
    for (uint32_t k = 0; k < nb; k++) {
        const int c = check_cols(batches[k]);
        if (c < 0) return c;
        if (c && !outs[k]) return -EFAULT;
        if (batches[k]->n > (1u << 30)) return -E2BIG;
    }
    hipStream_t s = (hipStream_t)stream;
    CtxScope cx(s);
    std::lock_guard<std::mutex> ag(a->mu);
    MapLocks L;
    lock_array_maps(L, a);
    L.lock();
    CallOrder co(s, L, a.get());
    PipeSync &P = pipe_sync();
    int r;
    if ((r = P.init())) return r;
    std::vector<std::shared_ptr<ProgLxc>> progs;
    if ((r = prog_table(a, s, progs))) return r;          // the program table k_ing_pack reads, on s
    if (hip_ok(hipEventRecord(P.ready, s), "ready") || hip_ok(hipStreamWaitEvent(P.aux, P.ready, 0), "aux wait"))
        return -EIO;
    auto prep = [&](uint32_t k) -> int {                  // batch k's schedule on the aux stream, workspace k & 1
        const int slot = (int)(k & 1u);
        if (k >= 2 && hip_ok(hipStreamWaitEvent(P.aux, P.done[slot], 0), "aux wait done")) return -EIO;
        cur_ctx().ws_slot = slot;
        int rr = batches[k]->n ? ingress_prepare(a, batches[k], P.aux) : 0;
        cur_ctx().ws_slot = 0;
        if (rr) return rr;
        return hip_ok(hipEventRecord(P.built[slot], P.aux), "built") ? -EIO : 0;
    };
    if (nb && (r = prep(0))) return r;
    for (uint32_t k = 0; k < nb; k++) {
        if (k + 1 < nb && (r = prep(k + 1))) return r;    // overlaps handle_policy of batch k
        const int slot = (int)(k & 1u);
        if (hip_ok(hipStreamWaitEvent(s, P.built[slot], 0), "wait built")) return -EIO;
        if (batches[k]->n) {
            cur_ctx().ws_slot = slot;
            PolicyPass pass;
            pass.out = outs[k];
            pass.prepared = true;                         // (prep(k) built the schedule)
            r = ingress_run(a, batches[k], now_sec[k], s, pass);
            cur_ctx().ws_slot = 0;
            if (r) return r;
        }
        if (hip_ok(hipEventRecord(P.done[slot], s), "done")) return -EIO;
    }
    return 0;
}

int gf_policy_ingress_classify(int array, const gf_pkt_cols *pkts, uint32_t now_sec, gf_ingress_out *out,
                               void *stream) {
    std::shared_lock<std::shared_mutex> g(prog_lock());
    auto a = get_as<PolicyArray>(array);
    if (!a) return -EBADF;
    int c = check_cols(pkts);
    if (c <= 0) return c;
    if (!out) return -EFAULT;
    if (pkts->n > (1u << 30)) return -E2BIG;
    CtxScope cx((hipStream_t)stream);
    std::lock_guard<std::mutex> ag(a->mu);
    MapLocks L;
    lock_array_maps(L, a);
    L.lock();
    CallOrder co((hipStream_t)stream, L, a.get());
    PolicyPass pass;
    pass.out = out;
    return ingress_run(a, pkts, now_sec, (hipStream_t)stream, pass);
}

// ---- full pipeline ----
int gf_pipeline_load(const gf_pipeline_cfg *cfg) {
    std::unique_lock<std::shared_mutex> g(prog_lock());
    if (!cfg) return -EFAULT;
    auto p = std::make_shared<ProgPipe>();
    p->cfg = *cfg;
    if (cfg->xdp_prog) {
        p->xdp = get_as<ProgXdp>(cfg->xdp_prog);
        if (!p->xdp) return -EBADF;
    }
    if (cfg->lb_prog) {
        p->lb = get_as<ProgLb>(cfg->lb_prog);
        if (!p->lb) return -EBADF;
    }
    auto m = get_map(cfg->netdev.lxc_map);
    if (!m) return -EBADF;
    if (!lxc_map_ok(*m)) return -EINVAL;
    p->lxc = m;
    // ENCAP_IFINDEX for the netdev stage is the node's: it must be defined, with a tunnel map to look up
    if ((cfg->netdev.flags & GF_NETDEV_F_ENCAP) && (!node_cfg().encap_ifindex || !node_map(2))) return -EINVAL;
    p->policy = get_as<PolicyArray>(cfg->policy_array);
    if (!p->policy) return -EBADF;
    return new_handle(p);
}

int gf_pipeline_classify(int pipe, const gf_pipe_batch *b, uint32_t now_sec, gf_pipeline_out *out,
                         uint8_t *nd6, uint8_t *snap_out, void *stream) {
    return gf_pipeline_classify_tunnel(pipe, b, now_sec, out, nd6, snap_out, nullptr, stream);
}

int gf_pipeline_classify_tunnel(int pipe, const gf_pipe_batch *b, uint32_t now_sec, gf_pipeline_out *out,
                                uint8_t *nd6, uint8_t *snap_out, uint32_t *tunnel_ip, void *stream) {
    std::shared_lock<std::shared_mutex> g(prog_lock());
    auto p = get_as<ProgPipe>(pipe);
    if (!p) return -EBADF;
    if (!b) return -EFAULT;
    const gf_frames &fr = b->frames;
    int r = frames_check(fr, out != nullptr);
    if (r <= 0) return r;
    hipStream_t s = (hipStream_t)stream;
    HostMarks hm;
    CtxScope cx(s);
    std::lock_guard<std::mutex> ag(p->policy->mu);
    MapLocks L;
    if (p->xdp) lock_xdp_maps(L, *p->xdp);
    if (p->lb) { L.add(p->lb->lb4); L.add(p->lb->lb6); }
    L.add(p->lxc);
    lock_array_maps(L, p->policy);
    L.lock();
    CallOrder co(s, L, p->policy.get());
    PipeDev P{};
    if (p->xdp) {
        auto &x = *p->xdp;
        if ((r = push_map(x.m4h, s)) || (r = push_map(x.m4l, s)) || (r = push_map(x.m6h, s)) ||
            (r = push_map(x.m6l, s)) || (r = push_map(x.lxc, s)))
            return r;
        if (x.m4h) { P.x.h4 = x.m4h->hdesc(); P.x.has_h4 = 1; }
        if (x.m6h) { P.x.h6 = x.m6h->hdesc(); P.x.has_h6 = 1; }
        if (x.m4l) P.x.l4 = x.m4l->tdesc();
        if (x.m6l) P.x.l6 = x.m6l->tdesc();
        P.x.lxc = x.lxc->hdesc();
        xdp_sets(x.m4h, x.lxc, P.x, s);
        xdp_dir(x.m4l, P.x, s);
        P.has_xdp = 1;
    }
    if (p->lb) {
        if ((r = push_map(p->lb->lb4, s)) || (r = push_map(p->lb->lb6, s))) return r;
        P.L = lb_dev(*p->lb);
        P.lb_redirect_ifindex = p->lb->cfg.redirect_ifindex;
        P.has_lb = 1;
    }
    if ((r = push_map(p->lxc, s))) return r;
    const gf_netdev_cfg &nd = p->cfg.netdev;
    P.nd.lx = lxc_dev(p->lxc, s);
    P.nd.flags = nd.flags;
    P.nd.fixed_secctx = nd.fixed_secctx;
    memcpy(P.nd.router6, nd.router_ip6, 8);
    // GF_NETDEV_F_HANDLE_NS / _ENCAP: k_nd_front; neither set: k_pipe_front
    const bool ndx = nd.flags & (GF_NETDEV_F_HANDLE_NS | GF_NETDEV_F_ENCAP);
    NdxDev X{};
    if (ndx) {
        memcpy(X.router6, nd.router_ip6, 16);
        X.tunnel_ip = tunnel_ip;
        if (nd.flags & GF_NETDEV_F_ENCAP) {
            const gf_node_cfg &node = node_cfg();
            auto tun = node_map(2);
            if (!tun || !node.encap_ifindex) return -EINVAL;   // the node was reconfigured since gf_pipeline_load
            if ((r = push_map(tun, s))) return r;
            X.enc = encap_dev(node, tun, s);
        }
    } else if (tunnel_ip) {
        if (hip_ok(hipMemsetAsync(tunnel_ip, 0, (size_t)fr.n * 4, s), "tunnel_ip")) return -EIO;
    }
    PolicyPass pass;
    const uint32_t trace = (nd.flags & GF_NETDEV_F_TRACE_NOTIFY) ? (TR_FROM_STACK | (GF_STAGE_NETDEV << 8)) : 0u;
    return front_call(p->policy, fr, b->flow_hash, now_sec, out, snap_out, s, pass, trace, nd.ingress_ifindex, P.vec_copy,
                      P.tcap_in, ndx ? "k_nd_front" : "k_pipe_front",
                      [&](const FrontLaunch &f, const uint16_t *slot_of, gf_rec *rec, uint32_t *keys) {
        if (ndx)
            launch_nt(k_nd_front<256>, k_nd_front<128>, f, fr, b->tc_index, b->flow_hash, P, X, slot_of, rec, keys, f.s6,
                      f.d6, out, nd6, snap_out, f.sink, f.K);
        else
            launch_nt(k_pipe_front<256>, k_pipe_front<128>, f, fr, b->tc_index, b->flow_hash, P, slot_of, rec, keys, f.s6,
                      f.d6, out, nd6, snap_out, f.sink, f.K);
    });
}

// ---- bpf_lb over frames ----
int gf_lb_prog_set_dstmac(int prog, const uint8_t mac[6]) {
    std::unique_lock<std::shared_mutex> g(prog_lock());
    auto p = get_as<ProgLb>(prog);
    if (!p) return -EBADF;
    if (!(p->cfg.flags & GF_LB_F_REDIRECT)) return -EINVAL;   // LB_DSTMAC sits inside #ifdef LB_REDIRECT
    p->has_dstmac = mac != nullptr;
    if (mac) memcpy(p->dstmac, mac, 6); else memset(p->dstmac, 0, 6);
    return 0;
}

int gf_lb_classify_frames(int prog, const gf_frames *frames, const uint32_t *flow_hash, gf_lb_out *out,
                          uint8_t *nd6, uint8_t *snap_out, void *stream) {
    std::shared_lock<std::shared_mutex> g(prog_lock());
    auto p = get_as<ProgLb>(prog);
    if (!p) return -EBADF;
    if (!frames) return -EFAULT;
    const gf_frames &fr = *frames;
    int r = frames_check(fr, out != nullptr);
    if (r <= 0) return r;
    hipStream_t s = (hipStream_t)stream;
    CtxScope cx(s);
    MapLocks ML;
    ML.add(p->lb4); ML.add(p->lb6);
    ML.lock();
    CallOrder co(s, ML);
    if ((r = push_map(p->lb4, s)) || (r = push_map(p->lb6, s))) return r;
    const LbDev L = lb_dev(*p);
    LbFrDev F{};
    if (p->has_dstmac) {
        F.has_mac = 1;
        memcpy(&F.mac_lo, p->dstmac, 4);
        F.mac_hi = (uint32_t)p->dstmac[4] | ((uint32_t)p->dstmac[5] << 8);
    }
    const FrontLaunch f = front_geometry(fr, snap_out, s, F.vec_copy);   // the fronts' tiles
    {
        ProfScope ps("k_lb_frames", s);
        launch_nt(k_lb_frames<256>, k_lb_frames<128>, f, fr, flow_hash, L, F, out, nd6, snap_out, f.sink);
        if ((r = hip_ok(hipGetLastError(), "k_lb_frames"))) return r;
    }
    // send_drop_notify_error's records (bpf_lb.c:194-195): the drop list of ev_list without a trace.
    // gf_lb_out has no stage byte; a SHOT record is zero past its reason, so byte 2 reads as
    // GF_STAGE_NONE, which ev_list gives the caller's record: zeros for source, labels and ifindex,
    // as for GF_STAGE_LB.
    EvSrc E{};
    E.recs = (const uint8_t *)out;
    E.stride = sizeof(gf_lb_out); E.act_off = 0; E.stage_off = 2;
    E.len = fr.len; E.flow_hash = flow_hash; E.n = fr.n;
    E.snap = snap_out ? snap_out : fr.snap; E.snap_stride = fr.snap_stride;
    return emit_drop_events(E, s);
}

// ---- from-overlay ----
int gf_overlay_load(const gf_overlay_cfg *cfg) {
    std::unique_lock<std::shared_mutex> g(prog_lock());
    if (!cfg) return -EFAULT;
    auto p = std::make_shared<ProgOverlay>();
    p->cfg = *cfg;
    auto m = get_map(cfg->lxc_map);
    if (!m) return -EBADF;
    if (!lxc_map_ok(*m)) return -EINVAL;
    p->lxc = m;
    p->policy = get_as<PolicyArray>(cfg->policy_array);
    if (!p->policy) return -EBADF;
    return new_handle(p);
}

// gf_overlay_classify (with_opts false: a Geneve program is refused) and gf_overlay_classify_opts.
static int overlay_call(int ovl, const gf_overlay_batch *b, const gf_tunnel_opts *opts, bool with_opts,
                        uint32_t now_sec, gf_pipeline_out *out, uint8_t *snap_out, void *stream) {
    std::shared_lock<std::shared_mutex> g(prog_lock());
    auto p = get_as<ProgOverlay>(ovl);
    if (!p) return -EBADF;
    if (!b) return -EFAULT;
    const bool geneve = p->cfg.flags & GF_OVERLAY_F_GENEVE;
    if (geneve && !with_opts) return -EINVAL;          // ENCAP_GENEVE reads options: gf_overlay_classify_opts
    const gf_frames &fr = b->frames;
    int r = frames_check(fr, out && b->tunnel_id);
    if (r <= 0) return r;
    OvlOpt<true> G{};
    if (geneve) {                                      // a VXLAN program ignores opts
        if (!opts || !opts->opt || !opts->opt_len) return -EFAULT;
        if (opts->opt_stride < 4 || opts->opt_stride > 64 || (opts->opt_stride & 3u) || ((uintptr_t)opts->opt & 3u))
            return -EINVAL;
        G.opt = opts->opt; G.len = opts->opt_len; G.stride = opts->opt_stride;
    }
    hipStream_t s = (hipStream_t)stream;
    HostMarks hm;
    CtxScope cx(s);
    std::lock_guard<std::mutex> ag(p->policy->mu);
    MapLocks L;
    L.add(p->lxc);
    lock_array_maps(L, p->policy);
    L.lock();
    CallOrder co(s, L, p->policy.get());
    OvlDev O{};
    if ((r = push_map(p->lxc, s))) return r;
    O.lx = lxc_dev(p->lxc, s);
    const gf_node_cfg &node = node_cfg();
    O.host_ifindex = node.host_ifindex;
    memcpy(O.host_mac, node.host_mac, 6); memcpy(O.node_mac, node.node_mac, 6);
    PolicyPass pass;
    const uint32_t trace = (p->cfg.flags & GF_OVERLAY_F_TRACE_NOTIFY) ? (TR_FROM_OVERLAY | (GF_STAGE_OVERLAY << 8)) : 0u;
    return front_call(p->policy, fr, b->flow_hash, now_sec, out, snap_out, s, pass, trace, p->cfg.ingress_ifindex, O.vec_copy,
                      O.tcap_in, "k_ovl_front",
                      [&](const FrontLaunch &f, const uint16_t *slot_of, gf_rec *rec, uint32_t *keys) {
        if (geneve)
            launch_nt(k_ovl_front<256, true>, k_ovl_front<128, true>, f, fr, b->tunnel_id, b->tc_index, O, slot_of, rec,
                      keys, f.s6, f.d6, out, snap_out, f.sink, f.K, G);
        else
            launch_nt(k_ovl_front<256, false>, k_ovl_front<128, false>, f, fr, b->tunnel_id, b->tc_index, O, slot_of, rec,
                      keys, f.s6, f.d6, out, snap_out, f.sink, f.K, OvlOpt<false>{});
    });
}

int gf_overlay_classify(int ovl, const gf_overlay_batch *b, uint32_t now_sec, gf_pipeline_out *out,
                        uint8_t *snap_out, void *stream) {
    return overlay_call(ovl, b, nullptr, false, now_sec, out, snap_out, stream);
}

int gf_overlay_classify_opts(int ovl, const gf_overlay_batch *b, const gf_tunnel_opts *opts, uint32_t now_sec,
                             gf_pipeline_out *out, uint8_t *snap_out, void *stream) {
    return overlay_call(ovl, b, opts, true, now_sec, out, snap_out, stream);
}

// ---- encap_and_redirect's tunnel metadata of an egress call's records ----
int gf_lxc_egress_tunnel_meta(int policy_array, const uint16_t *lxc_id, const gf_egress_out *records, uint32_t n,
                              uint32_t *tunnel_id, uint8_t *opt, uint8_t *opt_len, void *stream) {
    std::shared_lock<std::shared_mutex> g(prog_lock());
    auto a = get_as<PolicyArray>(policy_array);
    if (!a) return -EBADF;
    if (n == 0) return 0;
    if (!lxc_id || !records || !tunnel_id || !opt || !opt_len) return -EFAULT;
    if ((uintptr_t)opt & 3u) return -EINVAL;           // written as two words per packet (gf_tunnel_opts' alignment)
    if (n > (1u << 30)) return -E2BIG;
    hipStream_t s = (hipStream_t)stream;
    CtxScope cx(s);
    std::lock_guard<std::mutex> ag(a->mu);
    MapLocks L;                                        // prog_table pushes the programs' maps
    lock_array_maps(L, a);
    L.lock();
    CallOrder co(s, L, a.get());
    int r;
    std::vector<std::shared_ptr<ProgLxc>> progs;
    if ((r = prog_table(a, s, progs))) return r;
    ProfScope ps("k_tun_meta", s);
    hipLaunchKernelGGL(k_tun_meta, dim3((n + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, s, lxc_id, records, n,
                       (const uint16_t *)a->d_slot_of_lxc.p, (const gf_lxc_dev *)a->d_cfgs.p, tunnel_id,
                       reinterpret_cast<uint32_t *>(opt), opt_len);
    return hip_ok(hipGetLastError(), "k_tun_meta");
}

// ---- from-host ----
int gf_host_load(const gf_host_cfg *cfg) {
    std::unique_lock<std::shared_mutex> g(prog_lock());
    if (!cfg) return -EFAULT;
    auto p = std::make_shared<ProgHost>();
    p->cfg = *cfg;
    auto m = get_map(cfg->netdev.lxc_map);
    if (!m) return -EBADF;
    if (!lxc_map_ok(*m)) return -EINVAL;
    p->lxc = m;
    p->policy = get_as<PolicyArray>(cfg->policy_array);
    if (!p->policy) return -EBADF;
    return new_handle(p);
}

int gf_host_classify(int host, const gf_host_batch *b, uint32_t now_sec, gf_pipeline_out *out,
                     uint8_t *snap_out, void *stream) {
    std::shared_lock<std::shared_mutex> g(prog_lock());
    auto p = get_as<ProgHost>(host);
    if (!p) return -EBADF;
    if (!b) return -EFAULT;
    const gf_frames &fr = b->frames;
    int r = frames_check(fr, out != nullptr);
    if (r <= 0) return r;
    hipStream_t s = (hipStream_t)stream;
    HostMarks hm;
    CtxScope cx(s);
    std::lock_guard<std::mutex> ag(p->policy->mu);
    // cilium_proxy{4,6}, the tunnel map and the node's cilium_lxc are among the array's
    // maps: the front reads them under the locks ingress_run writes them under
    MapLocks L;
    L.add(p->lxc);
    lock_array_maps(L, p->policy);
    L.lock();
    CallOrder co(s, L, p->policy.get());
    HostDev H{};
    auto px4 = proxy_map(4), px6 = proxy_map(6), tun = node_map(2);
    if ((r = push_map(p->lxc, s)) || (r = push_map(px4, s)) || (r = push_map(px6, s)) || (r = push_map(tun, s))) return r;
    const gf_netdev_cfg &nd = p->cfg.netdev;
    H.lx = lxc_dev(p->lxc, s);
    H.enc = encap_dev(node_cfg(), tun, s);
    if (px4) H.px4 = px4->hdesc();
    if (px6) H.px6 = px6->hdesc();
    H.flags = nd.flags; H.fixed_secctx = nd.fixed_secctx;
    memcpy(H.router6, nd.router_ip6, 8);
    memcpy(H.net_mac, p->cfg.cilium_net_mac, 6);
    PolicyPass pass;
    pass.keep_flags = true;
    pass.hmark = b->mark;
    const uint32_t trace = (nd.flags & GF_NETDEV_F_TRACE_NOTIFY) ? (TR_FROM_HOST | (GF_STAGE_HOST << 8)) : 0u;
    return front_call(p->policy, fr, b->flow_hash, now_sec, out, snap_out, s, pass, trace, nd.ingress_ifindex, H.vec_copy,
                      H.tcap_in, "k_host_front",
                      [&](const FrontLaunch &f, const uint16_t *slot_of, gf_rec *rec, uint32_t *keys) {
        launch_nt(k_host_front<256>, k_host_front<128>, f, fr, b->mark, b->tc_index, H, slot_of, rec, keys, f.s6, f.d6, out,
                  snap_out, f.sink, f.K);
    });
}

// ---- ingest re-partition ----
int gf_pipeline_partition(int pipe, const gf_pipe_batch *b, uint32_t self_rank, uint32_t nranks, uint32_t *owner,
                          uint32_t *order, uint32_t *counts, void *stream) {
    std::shared_lock<std::shared_mutex> g(prog_lock());
    auto p = get_as<ProgPipe>(pipe);
    if (!p) return -EBADF;
    if (!b || !owner || !order || !counts) return -EFAULT;
    if (nranks == 0 || nranks > 65536 || self_rank >= nranks) return -EINVAL;
    const gf_frames &fr = b->frames;
    hipStream_t s = (hipStream_t)stream;
    CtxScope cx(s);
    MapLocks L;
    if (p->lb) { L.add(p->lb->lb4); L.add(p->lb->lb6); }
    L.lock();
    CallOrder co(s, L);
    if (hip_ok(hipMemsetAsync(counts, 0, (size_t)nranks * 4, s), "partition counts")) return -EIO;
    if (fr.n == 0) return 0;
    if (!fr.snap || !fr.len) return -EFAULT;
    if (fr.snap_stride < 14) return -EINVAL;
    if (fr.n > (1u << 30)) return -E2BIG;
    int r;
    PipeDev P{};
    if (p->lb) {
        if ((r = push_map(p->lb->lb4, s)) || (r = push_map(p->lb->lb6, s))) return r;
        P.L = lb_dev(*p->lb);
        P.has_lb = 1;
    }
    const uint32_t n = fr.n;
    struct PartWs { DevBuf keys, tmp; };
    static const char tag = 0;
    PartWs &pw = cur_ctx().get<PartWs>(&tag);
    DevBuf &keys = pw.keys, &tmp = pw.tmp;
    auto grow = [](DevBuf &d, size_t want) -> int { return d.bytes >= want ? 0 : d.ensure(want); };
    if ((r = grow(keys, (size_t)n * 4))) return r;
    {
        ProfScope ps("k_partition", s);
        hipLaunchKernelGGL(k_partition, dim3((n + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, s, fr, b->flow_hash, P, self_rank,
                           nranks, owner, counts);
        if ((r = hip_ok(hipGetLastError(), "k_partition"))) return r;
    }
    // stable counting order by owner: radix sort of (owner, index) over the owner's bits
    int bits = 1;
    while ((1u << bits) < nranks) bits++;
    size_t tb = 0;
    (void)rocprim::radix_sort_pairs(nullptr, tb, owner, (uint32_t *)keys.p, rocprim::counting_iterator<uint32_t>(0u), order,
                                    n, 0, bits, s);
    if ((r = grow(tmp, tb + 256))) return r;
    tb = tmp.bytes;
    if (hip_ok(rocprim::radix_sort_pairs(tmp.p, tb, owner, (uint32_t *)keys.p, rocprim::counting_iterator<uint32_t>(0u),
                                         order, n, 0, bits, s), "partition sort"))
        return -EIO;
    return 0;
}

// ---- conntrack GC ----
// The test gf_ct_gc and gf_ct_gc_maps apply to a handle's map: a CT map by its sizes.
static bool ct_gc_accepts(const Map &m) { return !m.is_lpm() && (m.ksz == 14 || m.ksz == 40) && m.vsz == 48; }
// A map whose host shadow is authoritative (the caller holds its lock): delete there, the
// replica is rebuilt on the next push.  Returns the entries deleted.
static bool ct_gc_on_host(const Map &m) { return m.host_valid || !m.dev_valid || !m.d_slots.p; }
static uint64_t ct_gc_host(Map &m, uint32_t filter_time) {
    if (m.ht.slots.empty()) return 0;                   // never materialised: no entries
    const uint32_t lt_off = m.ht.codec == GF_VCODEC_CT ? 0u : 32u;
    uint64_t dead = 0;
    std::vector<std::string> keys;
    uint8_t v[GF_CT_VSZ];
    for (uint64_t i = 0; i < m.ht.nslots; i++) {
        if (m.ht.state(i) != GF_SLOT_FULL) continue;
        m.ht.get_val(i, v);
        uint32_t lt;
        memcpy(&lt, v + lt_off, 4);
        if (lt < filter_time) keys.emplace_back((const char *)m.ht.key(i), m.ksz);
    }
    for (auto &k : keys) if (m.erase((const uint8_t *)k.data()) == 0) dead++;
    return dead;
}
int gf_ct_gc(int map, uint32_t filter_time, void *stream) {
    std::shared_lock<std::shared_mutex> g(prog_lock());
    auto m = get_map(map);
    if (!m) return -EBADF;
    if (!ct_gc_accepts(*m)) return -EINVAL;
    hipStream_t s = (hipStream_t)stream;
    CtxScope cx(s);
    std::lock_guard<std::recursive_mutex> mg(m->mu);
    CallOrder co(s, std::vector<OrderPt *>{&m->ord});
    if (ct_gc_on_host(*m)) return (int)std::min<uint64_t>(ct_gc_host(*m, filter_time), 0x7fffffff);
    LruDev *L;
    uint32_t *bits;
    int rr;
    if ((rr = ct_sweep_bufs(*m, L, bits))) return rr;
    GcCut cut{filter_time, filter_time, 1u, 0u};             // lifetime < filter_time
    const unsigned long long zero2[2] = {0, 0};
    if (hip_ok(hipMemcpyAsync(&L->cut, &cut, sizeof cut, hipMemcpyHostToDevice, s), "gc cut") ||
        hip_ok(hipMemcpyAsync(L->res, zero2, sizeof zero2, hipMemcpyHostToDevice, s), "gc res"))
        return -EIO;
    {
        ProfScope ps("k_gc", s);
        ct_sweep_launch(*m, L, bits, s);
    }
    if (hip_ok(hipGetLastError(), "k_gc")) return -EIO;
    unsigned long long r[2] = {0, 0};
    const GcCut off{0, 0, 0u, 0u};
    if (hip_ok(hipMemcpyAsync(r, L->res, 16, hipMemcpyDeviceToHost, s), "gc result") ||
        hip_ok(hipMemcpyAsync(&L->cut, &off, sizeof off, hipMemcpyHostToDevice, s), "gc cut off") ||
        hip_ok(hipStreamSynchronize(s), "gc sync"))
        return -EIO;
    // device element count: entries are deleted, tombstones were already uncounted
    uint32_t cnt = 0;
    if (hip_ok(hipMemcpy(&cnt, m->d_count.p, 4, hipMemcpyDeviceToHost), "gc count")) return -EIO;
    cnt = cnt >= r[0] ? cnt - (uint32_t)r[0] : 0u;
    if (hip_ok(hipMemcpy(m->d_count.p, &cnt, 4, hipMemcpyHostToDevice), "gc count")) return -EIO;
    m->dev_count_hi = cnt;
    m->ev_pending = 0;
    m->st_floor = m->lru_seq;
    m->device_modified();
    return (int)std::min<unsigned long long>(r[0], 0x7fffffff);
}

// One GC round over many CT maps (EnableConntrackGC, pkg/endpointmanager/conntrack.go:84-130:
// every endpoint's local pair and the global pair): the outcome of gf_ct_gc on each map,
// with one validation, one set of locks (MapLocks, address order), one CallOrder, and for
// the device-owned maps GF_GC_MULTI maps per chain of three launches (k_gc_*_multi), the
// counts fixed on the device and one readback of every map's result row.
int gf_ct_gc_maps(const int *maps, uint32_t n, uint32_t filter_time, uint32_t *deleted, void *stream) {
    if (n == 0) return 0;
    if (!maps) return -EFAULT;
    if (n > 65536u) return -E2BIG;
    std::shared_lock<std::shared_mutex> g(prog_lock());
    std::vector<std::shared_ptr<Map>> ms(n);
    for (uint32_t k = 0; k < n; k++) {
        if (!(ms[k] = get_map(maps[k]))) return -EBADF;
        if (!ct_gc_accepts(*ms[k])) return -EINVAL;
    }
    hipStream_t s = (hipStream_t)stream;
    CtxScope cx(s);
    MapLocks ml;
    for (auto &m : ms) ml.add(m);
    ml.lock();
    if (ml.held.size() != n) return -EINVAL;            // the same map object twice (lock() drops duplicates)
    CallOrder co(s, ml);
    // the device-owned maps' buffers first: a failure here has touched no map
    std::vector<uint32_t> dev;
    for (uint32_t k = 0; k < n; k++) {
        if (ct_gc_on_host(*ms[k])) continue;
        LruDev *L;
        uint32_t *bits;
        int rr;
        if ((rr = ct_sweep_bufs(*ms[k], L, bits))) return rr;
        dev.push_back(k);
    }
    struct GcWs { DevBuf res; std::vector<unsigned long long> h; };
    static const char tag = 0;
    GcWs &w = cur_ctx().get<GcWs>(&tag);
    const size_t row = 4 * sizeof(unsigned long long);
    if (!dev.empty() && w.res.bytes < dev.size() * row) {
        size_t cap = 64;
        while (cap < dev.size()) cap *= 2;
        if (w.res.ensure(cap * row)) return -ENOMEM;
    }
    std::vector<unsigned long long> cnt(n, 0ull);
    for (uint32_t k = 0; k < n; k++)
        if (ct_gc_on_host(*ms[k])) cnt[k] = ct_gc_host(*ms[k], filter_time);
    if (!dev.empty()) {
        unsigned long long *res = (unsigned long long *)w.res.p;
        if (hip_ok(hipMemsetAsync(res, 0, dev.size() * row, s), "gc rows")) return -EIO;
        {
            ProfScope ps("k_gc_multi", s);
            for (size_t b = 0; b < dev.size(); b += GF_GC_MULTI) {
                GcBatch B{};
                B.n = (uint32_t)std::min<size_t>(GF_GC_MULTI, dev.size() - b);
                uint64_t tiles = 0;
                for (uint32_t j = 0; j < B.n; j++) {
                    Map &m = *ms[dev[b + j]];
                    GcMap &M = B.m[j];
                    M.d = m.hdesc();
                    M.bits = (uint32_t *)m.d_gcbits.p;
                    M.res = res + 4 * (b + j);
                    M.mode = m.ht.mode;
                    M.lt_off = m.ht.codec == GF_VCODEC_CT ? 0u : 32u;
                    B.t0[j] = (uint32_t)tiles;
                    tiles += ((M.d.mask + 1 + 31) / 32 + BLOCK - 1) / BLOCK;
                }
                if (tiles > 0xffffffffull) return -E2BIG;   // (2^45 slots: no such tables)
                B.t0[B.n] = (uint32_t)tiles;
                const uint32_t grid = (uint32_t)std::min<uint64_t>(tiles, 65535u * 8);
                hipLaunchKernelGGL(k_gc_starts_multi, dim3(grid), dim3(BLOCK), 0, s, B);
                hipLaunchKernelGGL(k_gc_clusters_multi, dim3(grid), dim3(BLOCK), 0, s, B, filter_time);
                hipLaunchKernelGGL(k_gc_end_multi, dim3(1), dim3(64), 0, s, B);
            }
        }
        if (hip_ok(hipGetLastError(), "k_gc_multi")) return -EIO;
        w.h.resize(dev.size() * 4);
        if (hip_ok(hipMemcpyAsync(w.h.data(), res, dev.size() * row, hipMemcpyDeviceToHost, s), "gc rows back") ||
            hip_ok(hipStreamSynchronize(s), "gc sync"))
            return -EIO;
        for (size_t j = 0; j < dev.size(); j++) {
            Map &m = *ms[dev[j]];
            cnt[dev[j]] = w.h[4 * j];
            m.dev_count_hi = w.h[4 * j + 2];            // exact: k_gc_end_multi left the count there
            m.ev_pending = 0;
            m.st_floor = m.lru_seq;
            m.device_modified();
        }
    }
    unsigned long long sum = 0;
    for (uint32_t k = 0; k < n; k++) {
        sum += cnt[k];
        if (deleted) deleted[k] = (uint32_t)std::min<unsigned long long>(cnt[k], 0xffffffffull);
    }
    return (int)std::min<unsigned long long>(sum, 0x7fffffff);
}

// ---- proxy map GC / redirect-close cleanup ----
// Both states of a map, as gf_ct_gc: on the host shadow while it is authoritative (no
// launch, no device needed), else a sweep of the HBM replica.  After the sweep the
// device count drops by the entries deleted and the host's bound of it (dev_count_hi,
// which px_log_apply only ever raises) is that exact count, so the next proxy log is
// applied in parallel again whenever count + log <= max_entries.
static int px_gc(int map, const PxGcPred &pred_of_v4, const PxGcPred &pred_of_v6, void *stream) {
    std::shared_lock<std::shared_mutex> g(prog_lock());
    auto m = get_map(map);
    if (!m) return -EBADF;
    const bool v4 = m->ksz == 10 && m->vsz == 16, v6 = m->ksz == 22 && m->vsz == 28;
    if (m->is_lpm() || (!v4 && !v6)) return -EINVAL;
    const PxGcPred P = v4 ? pred_of_v4 : pred_of_v6;
    hipStream_t s = (hipStream_t)stream;
    CtxScope cx(s);
    std::lock_guard<std::recursive_mutex> mg(m->mu);
    CallOrder co(s, std::vector<OrderPt *>{&m->ord});
    if (m->host_valid || !m->dev_valid || !m->d_slots.p) {
        if (m->ht.slots.empty()) return 0;              // never materialised: no entries
        uint64_t dead = 0;
        std::vector<std::string> keys;
        uint8_t v[28];
        for (uint64_t i = 0; i < m->ht.nslots; i++) {
            if (m->ht.state(i) != GF_SLOT_FULL) continue;
            const uint8_t *k = m->ht.key(i);
            bool kill;
            if (P.mode == GF_PXGC_LIFETIME) {
                m->ht.get_val(i, v);
                uint32_t lt;
                memcpy(&lt, v + P.off, 4);
                kill = lt < P.arg;
            } else {
                uint16_t dp;
                memcpy(&dp, k + P.off, 2);
                kill = dp == P.arg && k[P.nh_off] == 6;
            }
            if (kill) keys.emplace_back((const char *)k, m->ksz);
        }
        for (auto &k : keys) if (m->erase((const uint8_t *)k.data()) == 0) dead++;
        return (int)std::min<uint64_t>(dead, 0x7fffffff);
    }
    struct PxGcWs { DevBuf st; };
    static const char tag = 0;
    DevBuf &st = cur_ctx().get<PxGcWs>(&tag).st;
    if (!st.p && st.ensure(sizeof(PxGcDev))) return -ENOMEM;
    const size_t nw = (m->ht.nslots + 31) / 32;
    if (m->d_gcbits.bytes < nw * 4 && m->d_gcbits.ensure(nw * 4)) return -ENOMEM;
    PxGcDev *D = (PxGcDev *)st.p;
    uint32_t *bits = (uint32_t *)m->d_gcbits.p;
    PxGcDev init{};
    init.on.active = 1u;
    if (hip_ok(hipMemcpyAsync(D, &init, sizeof init, hipMemcpyHostToDevice, s), "proxy gc init")) return -EIO;
    {
        ProfScope ps("k_px_gc", s);
        const gf_htab_desc d = m->hdesc();
        const uint32_t grid = (uint32_t)std::min<uint64_t>((nw + BLOCK - 1) / BLOCK, 65535u * 8);
        hipLaunchKernelGGL(k_gc_starts, dim3(grid), dim3(BLOCK), 0, s, d, bits, (const GcCut *)&D->on);
        hipLaunchKernelGGL(k_px_gc, dim3(grid), dim3(BLOCK), 0, s, d, P, (const uint32_t *)bits, D->res);
    }
    if (hip_ok(hipGetLastError(), "k_px_gc")) return -EIO;
    unsigned long long r[2] = {0, 0};
    if (hip_ok(hipMemcpyAsync(r, D->res, 16, hipMemcpyDeviceToHost, s), "proxy gc result") ||
        hip_ok(hipStreamSynchronize(s), "proxy gc sync"))
        return -EIO;
    uint32_t cnt = 0;
    int rr;
    if ((rr = m->dev_count(cnt))) return rr;
    cnt = cnt >= r[0] ? cnt - (uint32_t)r[0] : 0u;
    if ((rr = m->dev_set_count(cnt))) return rr;        // the device count and dev_count_hi, both exact
    m->device_modified();
    return (int)std::min<unsigned long long>(r[0], 0x7fffffff);
}

int gf_proxy_gc(int map, uint32_t filter_time, void *stream) {
    return px_gc(map, PxGcPred{GF_PXGC_LIFETIME, filter_time, 12u, 0u}, PxGcPred{GF_PXGC_LIFETIME, filter_time, 24u, 0u}, stream);
}

int gf_proxy_cleanup_port(int map, uint16_t dport, void *stream) {
    return px_gc(map, PxGcPred{GF_PXGC_PORT, dport, 4u, 8u}, PxGcPred{GF_PXGC_PORT, dport, 16u, 20u}, stream);
}

#if GF_WRSTATS
// Diagnostic builds only: the write-source counters (gf_device.h WR_*), read and cleared.
int gf_diag_wrstats(unsigned long long *out, uint32_t n) {
    if (hip_ok(hipDeviceSynchronize(), "wrstats sync")) return -EIO;
    unsigned long long v[WR_N] = {0};
    if (hip_ok(hipMemcpyFromSymbol(v, HIP_SYMBOL(g_wrstat), sizeof v), "wrstats")) return -EIO;
    const unsigned long long z[WR_N] = {0};
    if (hip_ok(hipMemcpyToSymbol(HIP_SYMBOL(g_wrstat), z, sizeof z), "wrstats clear")) return -EIO;
    for (uint32_t k = 0; k < n && k < WR_N; k++) out[k] = v[k];
    return WR_N;
}
#endif

int gf_ct_evict_log(int map, gf_ct_evict_rec *out, uint32_t max) {
    auto m = get_map(map);
    if (!m) return -EBADF;
    if (max && !out) return -EFAULT;
    std::lock_guard<std::recursive_mutex> mg(m->mu);
    if (!m->d_lru.p) return 0;
    static_assert(sizeof(LruLog) == sizeof(gf_ct_evict_rec), "log record layout");
    if (hip_ok(hipDeviceSynchronize(), "evict log sync")) return -EIO;
    uint32_t n = 0;
    LruDev *L = (LruDev *)m->d_lru.p;
    if (hip_ok(hipMemcpy(&n, &L->nlog, 4, hipMemcpyDeviceToHost), "evict log count")) return -EIO;
    const uint32_t k = std::min(std::min(n, GF_LRU_LOGCAP), max);
    if (k && hip_ok(hipMemcpy(out, L->log, (size_t)k * sizeof(LruLog), hipMemcpyDeviceToHost), "evict log")) return -EIO;
    return (int)std::min<uint32_t>(n, 0x7fffffffu);
}

}  // extern "C"
