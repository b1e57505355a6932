// gf_respond.h — the ARP / ICMPv6 responder tail calls (included at the end of
// gf_kernels.hip: kernels and the host side of gf_respond_load / gf_respond /
// gf_respond_calls).
//
//   CILIUM_CALL_ARP                      tail_handle_arp  bpf/bpf_lxc.c:692-696 -> arp_respond  lib/arp.h:34-95
//   CILIUM_CALL_HANDLE_ICMP6_NS          lib/icmp6.h:146-199, 331-361
//   CILIUM_CALL_SEND_ICMP6_ECHO_REPLY    lib/icmp6.h:84-127
//   CILIUM_CALL_SEND_ICMP6_TIME_EXCEEDED lib/icmp6.h:201-312 (HAVE_SKB_CHANGE_TAIL)
//
// k_respond: one lane per frame reads the call column (coalesced); the frames with
// a call are compacted per block (ballot + wave totals) into LDS rows, loaded and
// stored by the whole block, so a block without responder work touches no frame and
// the lanes that do run a call sit in the block's first waves.  The four calls still
// diverge inside those waves: they share icmp6_send_reply, and responder frames are
// a sliver of real traffic.
#pragma once

struct RespEnt { uint32_t mac[2], lxc_id, pad; };      // NODE_MAC (LE words) and LXC_ID of one endpoint program
struct RespDev {
    const uint16_t *slot_of;   // lxc_id -> entry + 1, 0 = empty slot (null with use_lxc: every slot is empty)
    const RespEnt *ents;
    uint32_t node_mac[2];      // gf_node_cfg.node_mac (the node's programs)
    uint32_t gw;               // IPV4_GATEWAY, raw be32
    uint32_t router[4];        // ROUTER_IP, LE words
    uint32_t flags, max_len, use_lxc, vec_copy;
};
#define D_UNKNOWN_TARGET (-150)

__device__ __forceinline__ uint32_t resp_mac_b(const uint32_t *m, uint32_t k) { return (m[k >> 2] >> (8 * (k & 3))) & 0xffu; }
__device__ __forceinline__ void resp_put_mac(Row &w, uint32_t off, const uint32_t *m) {
    for (uint32_t k = 0; k < 6; k++) w.w8(off + k, resp_mac_b(m, k));
}
__device__ __forceinline__ void resp_get_mac(const Row &w, uint32_t off, uint32_t *m) {
    m[0] = w.r32(off); m[1] = w.r16(off + 4);
}
// bpf_csum_diff(from, 4 * nw, to, 4 * nw, seed)
__device__ __forceinline__ uint32_t resp_diff(const uint32_t *from, const uint32_t *to, int nw) {
    uint32_t s = 0;
    for (int k = 0; k < nw; k++) s = ck_add(s, ~from[k]);
    for (int k = 0; k < nw; k++) s = ck_add(s, to[k]);
    return s;
}

// arp_respond (lib/arp.h:67-95): direct packet access, so one bound check for the whole header
__device__ int resp_arp(const RespDev &R, Row &w, uint32_t len, const uint32_t *mac) {
    if (len < 42) return TC_OK;                         // :76
    uint32_t dm[2], sm[2];
    resp_get_mac(w, 0, dm); resp_get_mac(w, 6, sm);
    const bool bcast = dm[0] == 0xffffffffu && dm[1] == 0xffffu;
    const bool own = dm[0] == mac[0] && dm[1] == (mac[1] & 0xffffu);
    // arp_check (:35-45): ar_op 20, ar_hrd 14, ar_tip 38
    if (w.r16(20) != 0x0100u || w.r16(14) != 0x0100u || !(bcast || own) || w.r32(38) != R.gw) return TC_OK;
    const uint32_t sip = w.r32(28);
    resp_put_mac(w, 6, mac);                            // arp_prepare_response (:47-65)
    resp_put_mac(w, 0, sm);
    w.w16(20, 0x0200u);
    resp_put_mac(w, 22, mac);
    w.w32(28, R.gw);
    resp_put_mac(w, 32, sm);
    w.w32(38, sip);
    return TC_REDIRECT;
}

// icmp6_send_reply (lib/icmp6.h:43-82)
__device__ int resp_icmp6_reply(const RespDev &R, Row &w, uint32_t len, const uint32_t *mac) {
    if (!skb_ok(22, 16, len) || !skb_ok(38, 16, len)) return D_INVALID;
    uint32_t sip[4], dip[4];
    for (int k = 0; k < 4; k++) { sip[k] = w.r32(22 + 4 * k); dip[k] = w.r32(38 + 4 * k); }
    for (int k = 0; k < 4; k++) w.w32(22 + 4 * k, R.router[k]);
    for (int k = 0; k < 4; k++) w.w32(38 + 4 * k, sip[k]);
    if (l4_csum(w, len, 56, 0, resp_diff(sip, R.router, 4), GF_F_PSEUDO_HDR) < 0) return D_CSUM_L4;
    if (l4_csum(w, len, 56, 0, resp_diff(dip, sip, 4), GF_F_PSEUDO_HDR) < 0) return D_CSUM_L4;
    if (!skb_ok(6, 6, len)) return D_INVALID;
    uint32_t sm[2];
    resp_get_mac(w, 6, sm);
    resp_put_mac(w, 0, sm);
    resp_put_mac(w, 6, mac);
    return TC_REDIRECT;
}

// the 8-byte ICMPv6 header at 54 replaced by {type, 0, old checksum, w1} (send_icmp6_ndisc_adv :154-174,
// __icmp6_send_echo_reply :92-113)
__device__ int resp_icmp6_hdr(Row &w, uint32_t len, uint32_t type, bool keep_w1, uint32_t w1) {
    if (!skb_ok(54, 8, len)) return D_INVALID;
    const uint32_t o[2] = {w.r32(54), w.r32(58)};
    const uint32_t nw[2] = {type | (o[0] & 0xffff0000u), keep_w1 ? o[1] : w1};
    w.w32(54, nw[0]); w.w32(58, nw[1]);
    if (l4_csum(w, len, 56, 0, resp_diff(o, nw, 2), GF_F_PSEUDO_HDR) < 0) return D_CSUM_L4;
    return 0;
}

// __icmp6_handle_ns -> send_icmp6_ndisc_adv (lib/icmp6.h:331-350, 146-199)
__device__ int resp_ns(const RespDev &R, Row &w, uint32_t len, const uint32_t *mac) {
    if (!skb_ok(62, 16, len)) return D_INVALID;
    bool eq = true;
    for (int k = 0; k < 4; k++) eq &= w.r32(62 + 4 * k) == R.router[k];
    if (!eq) return (R.flags & GF_RESPOND_F_NS_TO_STACK) ? TC_OK : D_UNKNOWN_TARGET;
    // icmp6_router = 1, icmp6_solicited = 1, icmp6_override = 0: bits 7, 6, 5 of byte 58
    // (little-endian bitfield of linux/icmpv6.h: reserved:5, override:1, solicited:1, router:1)
    int r = resp_icmp6_hdr(w, len, 136u, false, 0xC0u);
    if (r) return r;
    if (!skb_ok(78, 8, len)) return D_INVALID;
    const uint32_t o[2] = {w.r32(78), w.r32(82)};
    const uint32_t nw[2] = {2u | (1u << 8) | (resp_mac_b(mac, 0) << 16) | (resp_mac_b(mac, 1) << 24),
                            resp_mac_b(mac, 2) | (resp_mac_b(mac, 3) << 8) | (resp_mac_b(mac, 4) << 16) |
                                (resp_mac_b(mac, 5) << 24)};
    w.w32(78, nw[0]); w.w32(82, nw[1]);
    if (l4_csum(w, len, 56, 0, resp_diff(o, nw, 2), GF_F_PSEUDO_HDR) < 0) return D_CSUM_L4;
    return resp_icmp6_reply(R, w, len, mac);
}

// __icmp6_send_time_exceeded (lib/icmp6.h:217-296); len becomes skb->len after skb_change_tail
__device__ int resp_time_exceeded(const RespDev &R, Row &w, uint32_t &len, uint32_t S, const uint32_t *mac) {
    uint32_t d[17];                                     // data[]: icmp6hdr 8, the IPv6 header 40, upper 8 / 20
    d[0] = 3u; d[1] = 0u;
    if (!skb_ok(14, 40, len)) return D_INVALID;
#pragma unroll
    for (int k = 0; k < 10; k++) d[2 + k] = w.r32(14 + 4 * k);
    w.w8(20, 58u);                                      // ipv6_store_nexthdr
    const uint32_t nh = (d[3] >> 16) & 0xffu;
    const uint32_t un = (nh == 58u || nh == 17u) ? 2u : nh == 6u ? 5u : 0u;
    if (!un) return D_UNKNOWN_L4;
    if (!skb_ok(54, 4 * un, len)) return D_INVALID;
#pragma unroll
    for (uint32_t k = 0; k < 5; k++) d[12 + k] = k < un ? w.r32(54 + 4 * k) : 0u;
    const uint32_t plen = 48u + 4u * un;                // 56 / 68
    uint32_t sum = 0;                                   // compute_icmp6_csum (:201-214)
#pragma unroll
    for (int k = 0; k < 17; k++) sum = ck_add(sum, d[k]);   // words past the payload are 0
#pragma unroll
    for (int k = 4; k < 12; k++) sum = ck_add(sum, d[k]);   // ipv6_pseudohdr_checksum: the original addresses,
    sum = ck_add(sum, plen << 24);                          // htonl(payload_len), htonl(IPPROTO_ICMPV6)
    sum = ck_add(sum, 58u << 24);
    const uint32_t pl = ((d[3] & 0xffu) << 8) | ((d[3] >> 8) & 0xffu);
    const uint32_t new_len = len + plen - pl;           // u32 + int, as skb->len + trimlen
    if (new_len < 54u || new_len > R.max_len) return D_WRITE_ERROR;   // skb_change_tail
    for (uint32_t k = len < new_len ? len : new_len; k < S; k++) w.p[k] = 0;
    len = new_len;
    w.cap = S < len ? S : len;
    if (!skb_ok(54, plen, len)) return D_WRITE_ERROR;
#pragma unroll
    for (int k = 0; k < 17; k++) if ((uint32_t)k < 12 + un) w.w32(54 + 4 * k, d[k]);
    w.w8(18, plen >> 8); w.w8(19, plen & 0xffu);        // ipv6_store_paylen
    if (l4_csum(w, len, 56, 0, sum, GF_F_PSEUDO_HDR) < 0) return D_CSUM_L4;
    return resp_icmp6_reply(R, w, len, mac);
}

template <int NT>
__global__ __launch_bounds__(NT) void k_respond(gf_frames fr, const uint8_t *call, const uint16_t *lxc_id, RespDev R,
                                                gf_respond_out *out, uint8_t *snap_out, uint32_t *blk_drops) {
    extern __shared__ uint4 lds_rows[];
    uint8_t *rows = reinterpret_cast<uint8_t *>(lds_rows);
    __shared__ uint16_t list[NT];
    __shared__ uint32_t wtot[NT / 64], drops;
    const uint32_t S = fr.snap_stride;
    const uint32_t b0 = blockIdx.x * NT, tid = threadIdx.x;
    const uint32_t i = b0 + tid;
    if (tid == 0) drops = 0;
    uint32_t c = 0, ent = 0;
    bool act = false;
    if (i < fr.n) {
        c = call[i];
        if (c) {
            bool miss = c > 4u;
            if (R.use_lxc) {
                ent = R.slot_of ? R.slot_of[lxc_id[i]] : 0u;
                miss |= ent == 0u;
            }
            act = !miss;
        }
    }
    const unsigned long long bal = __ballot(act);
    const uint32_t lane = tid & 63u, wv = tid >> 6;
    if (lane == 0) wtot[wv] = (uint32_t)__popcll(bal);
    __syncthreads();
    uint32_t base = 0, nact = 0;
    for (uint32_t k = 0; k < NT / 64; k++) { if (k < wv) base += wtot[k]; nact += wtot[k]; }
    if (act) list[base + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull))] = (uint16_t)tid;
    if (i < fr.n && !act) {                             // call 0, or the tail call into an empty slot
        gf_respond_out o{};
        o.call = (uint8_t)c; o.len = fr.len[i];
        if (c) { o.action = TC_SHOT; o.reason = 140; if (blk_drops) atomicAdd(&drops, 1u); }
        out[i] = o;
    }
    if (nact) {                                         // block-uniform
        __syncthreads();
        const uint32_t unit = R.vec_copy ? 16u : 1u, per = S / unit;
        for (uint32_t k = tid; k < nact * per; k += NT) {
            const uint32_t a = k / per, j = k - a * per;
            const uint8_t *src = fr.snap + (size_t)(b0 + list[a]) * S;
            if (R.vec_copy) lds_rows[(size_t)a * per + j] = reinterpret_cast<const uint4 *>(src)[j];
            else rows[(size_t)a * S + j] = src[j];
        }
        __syncthreads();
        if (tid < nact) {
            const uint32_t j = b0 + list[tid];
            const uint32_t cj = call[j];
            uint32_t len = fr.len[j];
            const uint32_t *mac = R.node_mac;
            if (R.use_lxc) mac = R.ents[R.slot_of[lxc_id[j]] - 1u].mac;
            Row w{rows + (size_t)tid * S, S < len ? S : len};
            int r;
            if (cj == GF_CALL_ARP) r = resp_arp(R, w, len, mac);
            else if (cj == GF_CALL_ICMP6_NS) r = resp_ns(R, w, len, mac);
            else if (cj == GF_CALL_ICMP6_ECHO_REPLY) {
                r = resp_icmp6_hdr(w, len, 129u, true, 0u);
                if (!r) r = resp_icmp6_reply(R, w, len, mac);
            } else r = resp_time_exceeded(R, w, len, S, mac);
            gf_respond_out o{};
            o.call = (uint8_t)cj; o.len = len;
            if (r < 0) { o.action = TC_SHOT; o.reason = (uint8_t)(-r); if (blk_drops) atomicAdd(&drops, 1u); }
            else o.action = (uint8_t)r;
            out[j] = o;
        }
        __syncthreads();
        for (uint32_t k = tid; k < nact * per; k += NT) {
            const uint32_t a = k / per, j = k - a * per;
            uint8_t *dst = snap_out + (size_t)(b0 + list[a]) * S;
            if (R.vec_copy) reinterpret_cast<uint4 *>(dst)[j] = lds_rows[(size_t)a * per + j];
            else dst[j] = rows[(size_t)a * S + j];
        }
    }
    if (blk_drops) {
        __syncthreads();
        if (tid == 0) blk_drops[blockIdx.x] = drops;
    }
}

// send_drop_notify_error of the calls (lib/drop.h:117-120): one struct drop_notify per SHOT record, in
// batch order at boff[block] + the block-local rank; labels, dst_id and ifindex 0, source = EVENT_SOURCE
// (LXC_ID in the endpoint's object, bpf_lxc.c:21; 0 in the node's programs), len_orig = skb->len at the
// error, the payload the frame as it stood then: the snap_out row, or the frame as passed for a missed
// tail call (whose row is not written).
template <int NT>
__global__ __launch_bounds__(NT) void k_respond_events(gf_frames fr, const uint16_t *lxc_id, const uint32_t *flow_hash,
                                                       RespDev R, const gf_respond_out *out, const uint8_t *snap_out,
                                                       const uint32_t *boff, gf_event_ring ring) {
    __shared__ uint32_t sc[NT];
    const uint32_t i = blockIdx.x * NT + threadIdx.x;
    gf_respond_out o{};
    if (i < fr.n) o = out[i];
    const uint32_t m = (i < fr.n && o.action == TC_SHOT) ? 1u : 0u;
    sc[threadIdx.x] = m;
    __syncthreads();
    for (uint32_t d = 1; d < NT; d <<= 1) {             // inclusive scan
        const uint32_t v = threadIdx.x >= d ? sc[threadIdx.x - d] : 0u;
        __syncthreads();
        sc[threadIdx.x] += v;
        __syncthreads();
    }
    if (!m) return;
    const uint64_t pos = (uint64_t)*ring.count + boff[blockIdx.x] + sc[threadIdx.x] - 1u;
    if (pos >= ring.capacity) return;                   // ring full: the record is lost
    uint32_t source = 0;
    if (R.use_lxc && R.slot_of) {
        const uint32_t e = R.slot_of[lxc_id[i]];
        if (e) source = R.ents[e - 1u].lxc_id & 0xffffu;
    }
    const uint8_t *pay = (o.reason == 140 ? fr.snap : snap_out) + (size_t)i * fr.snap_stride;
    const uint32_t cap = o.len < GF_TRACE_PAYLOAD_LEN ? o.len : GF_TRACE_PAYLOAD_LEN;
    uint32_t *w = reinterpret_cast<uint32_t *>(ring.records + pos * GF_EVENT_RECORD);
    w[0] = 1u /* CILIUM_NOTIFY_DROP */ | ((uint32_t)o.reason << 8) | (source << 16);
    w[1] = flow_hash ? flow_hash[i] : 0u;
    w[2] = o.len; w[3] = cap;
    w[4] = w[5] = w[6] = w[7] = 0u;
    for (uint32_t q = 0; q < GF_TRACE_PAYLOAD_LEN / 4; q++) {
        uint32_t v = 0;
        for (uint32_t b = 0; b < 4; b++) {
            const uint32_t off = 4 * q + b;
            if (off < cap && off < fr.snap_stride) v |= (uint32_t)pay[off] << (8 * b);
        }
        w[8 + q] = v;
    }
}

// The call column from the records of a classify call (gf_respond_calls).
__global__ __launch_bounds__(BLOCK) void k_respond_calls(gf_frames fr, const uint8_t *recs, uint32_t kind, uint8_t *call) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= fr.n) return;
    const uint8_t *r = recs + (size_t)i * 24;
    uint32_t c = GF_CALL_NONE;
    if (kind == GF_REC_EGRESS) {
        const uint32_t ef = *reinterpret_cast<const uint16_t *>(r + 14);    // gf_egress_out.eg_flags
        if (ef & GF_EG_F_ARP) c = GF_CALL_ARP;
        else if (ef & GF_EG_F_RESPONDER) {
            const uint32_t len = fr.len[i], cap = fr.snap_stride < len ? fr.snap_stride : len;
            c = fbyte(fr.snap + (size_t)i * fr.snap_stride, cap, 54) == 135u ? GF_CALL_ICMP6_NS : GF_CALL_ICMP6_ECHO_REPLY;
        } else if (ef & GF_EG_F_ICMP6_TE) c = GF_CALL_ICMP6_TIME_EXCEEDED;
    } else if (r[4] & GF_PIPE_F_ICMP6_TE) {                                 // gf_pipeline_out.flags
        c = GF_CALL_ICMP6_TIME_EXCEEDED;
    } else if (r[4] & GF_PIPE_F_RESPONDER) {                                // the netdev front's icmp6_handle
        c = r[5];                                                           // gf_pipeline_out.pad0
    }
    call[i] = (uint8_t)c;
}

// ---------------------------------------------------------------- host
namespace {
struct RespWs { DevBuf blk, boff, tmp; };
RespWs &resp_ws() { static const char tag = 0; return cur_ctx().get<RespWs>(&tag); }

// NODE_MAC / LXC_ID of the array's programs by slot, uploaded when the array changed.
int resp_table(ProgRespond &p, hipStream_t s) {
    PolicyArray &a = *p.policy;
    if (p.have_table && p.table_gen == a.gen) return 0;
    std::vector<uint16_t> slot_of(65536, 0);
    std::vector<RespEnt> ents;
    for (auto &kv : a.slots) {
        RespEnt e{};
        memcpy(e.mac, kv.second->cfg.node_mac, 6);
        e.lxc_id = kv.second->cfg.lxc_id;
        ents.push_back(e);
        slot_of[kv.first] = (uint16_t)ents.size();
    }
    int r;
    const size_t eb = std::max<size_t>(1, ents.size()) * sizeof(RespEnt);
    if (!p.d_slot_of.p && (r = p.d_slot_of.ensure(65536 * 2))) return r;
    if (p.d_ents.bytes < eb && (r = p.d_ents.ensure(eb))) return r;
    if (hip_ok(hipMemcpyAsync(p.d_slot_of.p, slot_of.data(), 65536 * 2, hipMemcpyHostToDevice, s), "responder slots"))
        return -EIO;
    if (!ents.empty() &&
        hip_ok(hipMemcpyAsync(p.d_ents.p, ents.data(), ents.size() * sizeof(RespEnt), hipMemcpyHostToDevice, s),
               "responder programs"))
        return -EIO;
    if (hip_ok(hipStreamSynchronize(s), "responder table")) return -EIO;
    p.table_gen = a.gen;
    p.have_table = true;
    return 0;
}
}  // namespace

extern "C" {

int gf_respond_load(const gf_respond_cfg *cfg) {
    std::unique_lock<std::shared_mutex> g(prog_lock());
    if (!cfg) return -EFAULT;
    if (cfg->flags & ~GF_RESPOND_F_NS_TO_STACK) return -EINVAL;
    auto p = std::make_shared<ProgRespond>();
    p->cfg = *cfg;
    if (cfg->policy_array) {
        p->policy = get_as<PolicyArray>(cfg->policy_array);
        if (!p->policy) return -EBADF;
    }
    return new_handle(p);
}

int gf_respond(int resp, const gf_respond_batch *b, gf_respond_out *out, uint8_t *snap_out, void *stream) {
    // prog_lock: the node config and the array's slots do not change under the call
    std::shared_lock<std::shared_mutex> g(prog_lock());
    auto p = get_as<ProgRespond>(resp);
    if (!p) return -EBADF;
    if (!b) return -EFAULT;
    const gf_frames &fr = b->frames;
    if (fr.n == 0) return 0;
    if (!fr.snap || !fr.len || !b->call || !out || !snap_out) return -EFAULT;
    if (fr.snap_stride < 122 || fr.snap_stride > 256) return -EINVAL;   // 14 + 40 + 68: the furthest byte a call touches
    if (snap_out == fr.snap) return -EINVAL;
    if (fr.n > (1u << 30)) return -E2BIG;
    hipStream_t s = (hipStream_t)stream;
    CtxScope cx(s);
    std::unique_lock<std::mutex> ag;
    if (p->policy) ag = std::unique_lock<std::mutex>(p->policy->mu);
    std::lock_guard<std::mutex> pg(p->mu);
    CallOrder co(s, std::vector<OrderPt *>{&p->ord});
    int r;
    const uint32_t n = fr.n;
    const gf_node_cfg &node = node_cfg();
    RespDev R{};
    memcpy(R.node_mac, node.node_mac, 6);
    R.gw = node.ipv4_gateway;
    memcpy(R.router, node.router_ip6, 16);
    R.flags = p->cfg.flags;
    R.max_len = p->cfg.max_len ? p->cfg.max_len : 1514u;
    R.use_lxc = b->lxc_id != nullptr;
    if (R.use_lxc && p->policy) {
        if ((r = resp_table(*p, s))) return r;
        R.slot_of = (const uint16_t *)p->d_slot_of.p;
        R.ents = (const RespEnt *)p->d_ents.p;
    }
    R.vec_copy = (fr.snap_stride % 16 == 0) && (((uintptr_t)fr.snap | (uintptr_t)snap_out) & 15u) == 0;
    // LDS rows as the fronts: 256 lanes per block up to 128-B snaps, 128 lanes up to 256 B (<= 32 KiB)
    const uint32_t nt = fr.snap_stride <= 128 ? 256u : 128u;
    const size_t lds = (size_t)nt * fr.snap_stride;
    const uint32_t grid = (n + nt - 1) / nt;
    const gf_event_ring ring = event_ring();
    const bool ev = ring.records && ring.count && ring.capacity;
    RespWs &w = resp_ws();
    auto grow = [](DevBuf &d, size_t want) -> int { return d.bytes >= want ? 0 : d.ensure(want); };
    size_t tb = 0;
    if (ev) {
        if ((r = grow(w.blk, (size_t)grid * 4)) || (r = grow(w.boff, (size_t)grid * 4))) return r;
        (void)rocprim::exclusive_scan(nullptr, tb, (uint32_t *)w.blk.p, (uint32_t *)w.boff.p, 0u, grid,
                                      rocprim::plus<uint32_t>(), s);
        if ((r = grow(w.tmp, tb + 256))) return r;
    }
    uint32_t *blk = ev ? (uint32_t *)w.blk.p : nullptr;
    {
        ProfScope ps("k_respond", s);
        if (nt == 256)
            hipLaunchKernelGGL(k_respond<256>, dim3(grid), dim3(256), lds, s, fr, b->call, b->lxc_id, R, out, snap_out, blk);
        else
            hipLaunchKernelGGL(k_respond<128>, dim3(grid), dim3(128), lds, s, fr, b->call, b->lxc_id, R, out, snap_out, blk);
        if ((r = hip_ok(hipGetLastError(), "k_respond"))) return r;
    }
    if (!ev) return 0;
    ProfScope ps("k_respond_events", s);
    tb = w.tmp.bytes;
    if (hip_ok(rocprim::exclusive_scan(w.tmp.p, tb, (uint32_t *)w.blk.p, (uint32_t *)w.boff.p, 0u, grid,
                                       rocprim::plus<uint32_t>(), s), "responder event scan"))
        return -EIO;
    if (nt == 256)
        hipLaunchKernelGGL(k_respond_events<256>, dim3(grid), dim3(256), 0, s, fr, b->lxc_id, b->flow_hash, R, out,
                           snap_out, (const uint32_t *)w.boff.p, ring);
    else
        hipLaunchKernelGGL(k_respond_events<128>, dim3(grid), dim3(128), 0, s, fr, b->lxc_id, b->flow_hash, R, out,
                           snap_out, (const uint32_t *)w.boff.p, ring);
    hipLaunchKernelGGL(k_ev_commit, dim3(1), dim3(1), 0, s, (const uint32_t *)w.boff.p, (const uint32_t *)w.blk.p, grid, ring);
    return hip_ok(hipGetLastError(), "k_respond_events");
}

int gf_respond_calls(const gf_frames *fr, const void *records, uint32_t rec_kind, uint8_t *call, void *stream) {
    if (!fr) return -EFAULT;
    if (rec_kind != GF_REC_EGRESS && rec_kind != GF_REC_PIPELINE) return -EINVAL;
    if (fr->n == 0) return 0;
    if (!records || !call || !fr->len || (rec_kind == GF_REC_EGRESS && !fr->snap)) return -EFAULT;
    if (fr->n > (1u << 30)) return -E2BIG;
    ProfScope ps("k_respond_calls", (hipStream_t)stream);
    hipLaunchKernelGGL(k_respond_calls, dim3((fr->n + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, (hipStream_t)stream, *fr,
                       (const uint8_t *)records, rec_kind, call);
    return hip_ok(hipGetLastError(), "k_respond_calls");
}

}  // extern "C"
