// gf_kernels.hip — gfx950 kernels of libgpuflow and the program/classify C ABI.
//
//   k_parse      raw frames -> SoA header columns   (skb_load_bytes rules)
//   k_xdp        bpf/bpf_xdp.c:88-184               one packet per lane
//   k_lb         bpf/bpf_lb.c:58-212 + lib/lb.h      one packet per lane
//   k_ing_pack   columns -> 32-B records + flow-group key (unordered addr pair)
//   (rocPRIM stable radix sort of (key, index); k_run_*: one bucket per run of equal keys)
//   k_bucket_*   bucket-size histogram + count-descending bucket order
//   k_ing_groups bpf/bpf_lxc.c:745-1024 handle_policy: a lane takes a flow-group bucket
//                off its family's queue and runs the bucket's packets in batch order
//                (CT ordering rule)
//   k_*_front    the frame entry points in front of it (pipeline, from-overlay, from-host)
//   k_eg_*       bpf/bpf_lxc.c:427-738 from-container
//
// Host side, in include-only headers, each included exactly once below:
//   gf_host_ctx.h       launch profiler, call contexts, check_cols, call order
//   gf_host_programs.h  gf_parse_frames, the program loads, gf_xdp_classify, gf_lb_classify
//   (between them and the next, in this file: PolicyPass, the flow-group schedule and k_run_*,
//   the CT sweeps, ingress_run)
//   gf_host_entry.h     the entry points over ingress_run, CT and proxy GC
//   gf_map_bulk.h       k_bulk_*, k_dump_gather: gf_map_update_batch, gf_map_lookup_batch
//   gf_host_egress.h    gf_lxc_egress_classify
#include "gf_internal.h"
#include "gf_device.h"
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/device/device_run_length_encode.hpp>
#include <rocprim/device/device_select.hpp>
#include <rocprim/iterator/discard_iterator.hpp>
#include <rocprim/iterator/counting_iterator.hpp>
#include <errno.h>
#include <stdlib.h>
#include <stdio.h>
#include <functional>
#include <unordered_set>
#include <chrono>
#include <algorithm>
#include <array>
#include <atomic>
#include <string.h>

using namespace gf;
using namespace gfd;

#define BLOCK 256
// Tuning knobs of the flow-group kernel (tools/variant.sh builds a library per setting).
// The bucket key (gf_key_cfg, gf_common.h: family bit + bits-1 bits of the group
// hash; GF_KEY_BITS forces a width, GF_SORT_RADIX sets the digit).
// The key of every packet the handle_policy pass skips (a pipeline packet that
// ended before the tail call, an egress packet that was not delivered locally):
// they sort into one run, which the bucket schedule leaves out, so no lane reads
// their records.  Group keys never take this value (gf_key_live).
__device__ __forceinline__ uint32_t gf_key_skip(const gf_key_cfg &K) { return K.hash; }
// h: a group hash (any 32 bits) -> its live family-0 key
__device__ __forceinline__ uint32_t gf_key_live(uint32_t h, const gf_key_cfg &K) {
    const uint32_t k = h & K.hash;
    return k == K.hash ? k - 1u : k;
}
#ifndef GF_ING_MINW
#define GF_ING_MINW 4       // __launch_bounds__ min waves per SIMD (register budget)
#endif
#ifndef GF_ING_MINW6
#define GF_ING_MINW6 3      // IPv6 buckets: the lane state (RelCache<10>) keeps the block at 3 per CU by LDS
#endif
#ifndef GF_EG_MINW
#define GF_EG_MINW 3        // k_eg_groups: min waves per SIMD (4 spills: 1.65 vs 1.60 ms, egress leg)
#endif
#ifndef GF_CT_COOP
#define GF_CT_COOP 1        // CT4 home lines read by complete lane quads together (ProbeLine::load_quad)
#endif
#ifndef GF_EG_COOP
#define GF_EG_COOP 1        // k_eg_groups: the CT4 home line read by complete lane quads (load_quad)
#endif
#ifndef GF_FRONT_MINW
#define GF_FRONT_MINW 8     // k_pipe_front: __launch_bounds__ min waves per SIMD (64 VGPRs: 1.294 vs 1.410 ms, config 4)
#endif
#define GF_RUN_ITEMS 4096u  // keys per tile of the run-start / single-bucket count-scan-write passes
// Buckets per lane per queue grab once a wave reaches the single-packet buckets
// (the lists are longest first, so from there on every bucket is one packet): one
// queue atomic per 64 x GF_GRAB_* buckets instead of per 64, and a lane runs several
// independent packets back to back.  Longer buckets keep one per lane per grab (a
// lane holding four long buckets would stretch the tail: config 2 4.8 vs 2.4 ms).
#ifndef GF_GRAB_ING
#define GF_GRAB_ING 4       // k_ing_groups
#endif
#ifndef GF_GRAB_EG
#define GF_GRAB_EG 2        // k_eg_groups
#endif
#ifndef GF_CT_COOP6
#define GF_CT_COOP6 1       // the same for CT6 (168 VGPRs: fits the 3 waves the LDS allows; 1.242 vs 1.252 ms)
#endif
#ifndef GF_MEMO4
#define GF_MEMO4 2          // policy decisions memoised per lane, IPv4 buckets
#endif
#ifndef GF_MEMO6
#define GF_MEMO6 2          // IPv6 buckets (1 fits 4 blocks' lane state in LDS, but the 128-VGPR
                            // budget that occupancy 4 then imposes spills: 1.93 vs 1.20 ms, config 5)
#endif

// ---------------------------------------------------------------- constants
enum {
    TC_OK = 0, TC_SHOT = 2, TC_REDIRECT = 7, XDP_DROP_ = 1, XDP_PASS_ = 2,
    D_POLICY = -133, D_INVALID = -134, D_CT_INVALID_HDR = -135, D_CT_UNKNOWN_PROTO = -137,
    D_UNKNOWN_L3 = -139, D_MISSED_TAIL_CALL = -140, D_WRITE_ERROR = -141, D_UNKNOWN_L4 = -142,
    D_CSUM_L4 = -154, D_CT_CREATE_FAILED = -155, D_NO_SERVICE = -158, D_POLICY_L4 = -159,
    D_NON_LOCAL = -151, D_NO_TUNNEL_OPT = -148, D_INVALID_GENEVE = -149,
};
enum { CT_NEW = 0, CT_ESTABLISHED = 1, CT_REPLY = 2, CT_RELATED = 3 };
enum { ACT_UNSPEC = 0, ACT_CREATE = 1, ACT_CLOSE = 2 };
#define F_RX_CLOSING 1u
#define F_TX_CLOSING 2u
#define F_LB_LOOPBACK 8u
#define F_SEEN_NON_SYN 16u

// ---------------------------------------------------------------- stats
struct Stats {
    uint32_t *lds;
    __device__ void init() {
        for (int k = threadIdx.x; k < 272; k += blockDim.x) lds[k] = 0;
        __syncthreads();
    }
    __device__ void add(uint32_t bin) { atomicAdd(&lds[bin], 1u); }
    __device__ void add_n(uint32_t bin, uint32_t v) { if (v) atomicAdd(&lds[bin], v); }
    // one packet: reason/action bins + packets, wire bytes, algorithmic bytes
    __device__ void pkt(uint32_t reason, uint32_t action, uint32_t len, uint32_t ab) {
        add(reason); add(256 + action); add(268); add_n(269, len); add_n(270, ab);
    }
    // pkt() aggregated over the wave: one LDS atomic per distinct (reason,
    // action) pair and one per sum instead of five per lane.  Every lane of the
    // wave must call it (act = the lane counts a packet; ab is summed over every
    // lane, so a lane without a packet passes 0).
    __device__ void pkt_wave(bool act, uint32_t reason, uint32_t action, uint32_t len, uint32_t ab) {
        uint32_t n = act ? 1u : 0u, l = act ? len : 0u, a = ab;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            n += __shfl_xor(n, o); l += __shfl_xor(l, o); a += __shfl_xor(a, o);
        }
        const uint32_t lane = threadIdx.x & 63u, key = (reason & 0xffu) | (action << 8);
        uint64_t rem = __ballot(act);
        while (rem) {
            const uint32_t lead = (uint32_t)__ffsll((unsigned long long)rem) - 1u;
            const uint32_t k = __shfl(key, (int)lead);
            const uint64_t m = __ballot(act && key == k) & rem;
            if (lane == lead) {
                atomicAdd(&lds[k & 0xffu], (uint32_t)__popcll(m));
                atomicAdd(&lds[256 + (k >> 8)], (uint32_t)__popcll(m));
            }
            rem &= ~m;
        }
        if (lane == 0) { if (n) { atomicAdd(&lds[268], n); atomicAdd(&lds[269], l); } if (a) atomicAdd(&lds[270], a); }
    }
    // pkt_wave's (reason, action) bins alone: for grid-stride loops that keep the
    // packet count and the byte sums per lane and hand them to sums() once
    __device__ void bins_wave(bool act, uint32_t reason, uint32_t action) {
        const uint32_t lane = threadIdx.x & 63u, key = (reason & 0xffu) | (action << 8);
        uint64_t rem = __ballot(act);
        while (rem) {
            const uint32_t lead = (uint32_t)__ffsll((unsigned long long)rem) - 1u;
            const uint32_t k = __shfl(key, (int)lead);
            const uint64_t m = __ballot(act && key == k) & rem;
            if (lane == lead) {
                atomicAdd(&lds[k & 0xffu], (uint32_t)__popcll(m));
                atomicAdd(&lds[256 + (k >> 8)], (uint32_t)__popcll(m));
            }
            rem &= ~m;
        }
    }
    __device__ void sums(uint32_t n, uint32_t len, uint32_t ab) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { n += __shfl_xor(n, o); len += __shfl_xor(len, o); ab += __shfl_xor(ab, o); }
        if ((threadIdx.x & 63u) == 0) { add_n(268, n); add_n(269, len); add_n(270, ab); }
    }
    // XDP verdict counts (reason 1 / XDP_DROP, reason 0 / XDP_PASS) and sums, summed
    // per lane over a whole grid-stride loop: one wave reduction (every lane calls it)
    __device__ void xdp_sums(uint32_t drop, uint32_t pass, uint32_t len, uint32_t ab) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            drop += __shfl_xor(drop, o); pass += __shfl_xor(pass, o);
            len += __shfl_xor(len, o); ab += __shfl_xor(ab, o);
        }
        if ((threadIdx.x & 63u) == 0) {
            add_n(1, drop); add_n(256 + 1, drop); add_n(0, pass); add_n(256 + 2, pass);
            add_n(268, drop + pass); add_n(269, len); add_n(270, ab);
        }
    }
    __device__ void flush(unsigned long long *g) {
        __syncthreads();
        for (int k = threadIdx.x; k < 272; k += blockDim.x)
            if (lds[k]) atomicAdd(&g[k], (unsigned long long)lds[k]);
    }
};

// ================================================================ parse
__device__ __forceinline__ uint32_t fbyte(const uint8_t *f, uint32_t cap, uint32_t off) {
    return off < cap ? f[off] : 0u;
}

// Header values of one frame, as the BPF programs hold them after their loads
// (the rules of gf_parse_frames; oracle.c o_parse_batch).
struct PktHdr {
    uint32_t et, sa, da, w0, w3, proto;
    int l4;
    uint32_t s6[4], d6[4];
};
__device__ __forceinline__ void parse_row(const uint8_t *f, uint32_t cap, uint32_t len, PktHdr &h) {
    h.et = len >= 14 ? ((fbyte(f, cap, 12) << 8) | fbyte(f, cap, 13)) : 0u;
    h.sa = h.da = h.w0 = h.w3 = h.proto = 0;
    h.l4 = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) h.s6[k] = h.d6[k] = 0;
    bool have = false;
    if (h.et == 0x0800 && len >= 34) {
        for (int k = 0; k < 4; k++) { h.sa |= fbyte(f, cap, 26 + k) << (8 * k); h.da |= fbyte(f, cap, 30 + k) << (8 * k); }
        h.proto = fbyte(f, cap, 23);
        h.l4 = 14 + (int)(fbyte(f, cap, 14) & 0xf) * 4;
        have = true;
    } else if (h.et == 0x86DD && len >= 54) {
        for (int k = 0; k < 16; k++) {
            h.s6[k >> 2] |= fbyte(f, cap, 22 + k) << (8 * (k & 3));
            h.d6[k >> 2] |= fbyte(f, cap, 38 + k) << (8 * (k & 3));
        }
        // ipv6_hdrlen, bpf/lib/ipv6.h:61-98 (AUTH length chosen by the NEXT header, as written)
        uint32_t nh = fbyte(f, cap, 20);
        int hl = 40, res = -156;
        for (int it = 0; it < 4; it++) {
            if (nh == 59) { res = -156; goto done; }
            if (nh == 44) { res = -157; goto done; }
            if (nh == 0 || nh == 43 || nh == 51 || nh == 60) {
                int off = 14 + hl;
                if (!skb_ok(off, 2, len)) { res = -134; goto done; }
                uint32_t onh = fbyte(f, cap, off), ohl = fbyte(f, cap, off + 1);
                nh = onh;
                if (nh == 51) hl += (int)(ohl + 2) << 2; else hl += (int)(ohl + 1) << 3;
                continue;
            }
            res = hl;
            h.proto = nh;
            goto done;
        }
        res = -156;
    done:
        if (res < 0) h.proto = fbyte(f, cap, 20);
        h.l4 = 14 + res;
        have = true;
    }
    if (have) {
        for (int k = 0; k < 4; k++) {
            int64_t off = (int64_t)h.l4 + k;
            if (off >= 0 && off < (int64_t)len) h.w0 |= fbyte(f, cap, (uint32_t)off) << (8 * k);
        }
        for (int k = 0; k < 2; k++) {
            int64_t off = (int64_t)h.l4 + 12 + k;
            if (off >= 0 && off < (int64_t)len) h.w3 |= fbyte(f, cap, (uint32_t)off) << (8 * k);
        }
    }
}

__global__ __launch_bounds__(BLOCK) void k_parse(gf_frames fr, gf_pkt_cols_out o) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < fr.n; i += gridDim.x * blockDim.x) {
        const uint8_t *f = fr.snap + (size_t)i * fr.snap_stride;
        uint32_t len = fr.len[i];
        uint32_t cap = fr.snap_stride < len ? fr.snap_stride : len;
        PktHdr h;
        parse_row(f, cap, len, h);
        o.ethertype[i] = (uint16_t)h.et; o.saddr4[i] = h.sa; o.daddr4[i] = h.da; o.proto[i] = (uint8_t)h.proto;
        o.l4_off[i] = (int16_t)h.l4; o.l4w0[i] = h.w0; o.l4w3[i] = (uint16_t)h.w3;
        if (o.saddr6) reinterpret_cast<uint4 *>(o.saddr6)[i] = make_uint4(h.s6[0], h.s6[1], h.s6[2], h.s6[3]);
        if (o.daddr6) reinterpret_cast<uint4 *>(o.daddr6)[i] = make_uint4(h.d6[0], h.d6[1], h.d6[2], h.d6[3]);
    }
}

// Header access for the per-packet programs: packet i of a column batch, or
// the values a lane parsed itself (the fused pipeline front).
struct ColA {
    const gf_pkt_cols &c;
    uint32_t i;
    __device__ __forceinline__ uint32_t saddr4() const { return c.saddr4[i]; }
    __device__ __forceinline__ uint32_t daddr4() const { return c.daddr4[i]; }
    __device__ __forceinline__ uint32_t proto() const { return c.proto[i]; }
    __device__ __forceinline__ int l4_off() const { return c.l4_off[i]; }
    __device__ __forceinline__ uint32_t l4w0() const { return c.l4w0[i]; }
    __device__ __forceinline__ uint32_t fhash() const { return c.flow_hash ? c.flow_hash[i] : 0u; }
    __device__ __forceinline__ bool has6() const { return c.saddr6 && c.daddr6; }
    __device__ __forceinline__ uint4 saddr6() const { return reinterpret_cast<const uint4 *>(c.saddr6)[i]; }
    __device__ __forceinline__ uint4 daddr6() const { return gload<uint4>(c.daddr6 + 16 * (size_t)i); }
};
struct PktHdrA {
    const PktHdr &h;
    uint32_t fh;
    __device__ __forceinline__ uint32_t saddr4() const { return h.sa; }
    __device__ __forceinline__ uint32_t daddr4() const { return h.da; }
    __device__ __forceinline__ uint32_t proto() const { return h.proto; }
    __device__ __forceinline__ int l4_off() const { return h.l4; }
    __device__ __forceinline__ uint32_t l4w0() const { return h.w0; }
    __device__ __forceinline__ uint32_t fhash() const { return fh; }
    __device__ __forceinline__ bool has6() const { return true; }
    __device__ __forceinline__ uint4 saddr6() const { return make_uint4(h.s6[0], h.s6[1], h.s6[2], h.s6[3]); }
    __device__ __forceinline__ uint4 daddr6() const { return make_uint4(h.d6[0], h.d6[1], h.d6[2], h.d6[3]); }
};
// The prefilter's three fields straight from a frame's row (k_xdpf_verdict): ethertype and
// the addresses under parse_row's rules, loaded when xdp_verdict asks for them; nothing else
// of PktHdr.  cap = min(len, snap_stride): a byte at or past it reads 0.  w4 / w6: the rows are
// 4-byte aligned and hold bytes [0, 36) / [0, 56), so the IPv4 / IPv6 addresses (all at offsets
// == 2 mod 4) come from whole dwords; xdp_verdict reads them only when len >= 34 / 54, and then
// every byte used lies below cap.
struct FrameA {
    const uint8_t *f;
    uint32_t cap;
    bool w4, w6;
    __device__ __forceinline__ uint32_t dw(uint32_t off) const { return *reinterpret_cast<const uint32_t *>(f + off); }
    __device__ __forceinline__ uint32_t mid(uint32_t off) const { return (dw(off - 2) >> 16) | (dw(off + 2) << 16); }
    __device__ __forceinline__ uint32_t b4(uint32_t off) const {
        return fbyte(f, cap, off) | (fbyte(f, cap, off + 1) << 8) | (fbyte(f, cap, off + 2) << 16) | (fbyte(f, cap, off + 3) << 24);
    }
    __device__ __forceinline__ uint32_t et(uint32_t len) const {
        return len >= 14 ? ((fbyte(f, cap, 12) << 8) | fbyte(f, cap, 13)) : 0u;
    }
    __device__ __forceinline__ uint32_t saddr4() const { return w4 ? mid(26) : b4(26); }
    __device__ __forceinline__ uint32_t daddr4() const { return w4 ? mid(30) : b4(30); }
    __device__ __forceinline__ bool has6() const { return true; }
    __device__ __forceinline__ uint4 saddr6() const {
        return w6 ? make_uint4(mid(22), mid(26), mid(30), mid(34)) : make_uint4(b4(22), b4(26), b4(30), b4(34));
    }
    __device__ __forceinline__ uint4 daddr6() const {
        return w6 ? make_uint4(mid(38), mid(42), mid(46), mid(50)) : make_uint4(b4(38), b4(42), b4(46), b4(50));
    }
};

// The lane's frame copy.  Reads past the snap (or len) are 0, writes past the
// snap are dropped (the snap holds every header byte the programs touch).
struct Row {
    uint8_t *p;
    uint32_t cap;
    __device__ __forceinline__ uint32_t b(uint32_t off) const { return off < cap ? (uint32_t)p[off] : 0u; }
    __device__ __forceinline__ uint32_t r16(uint32_t off) const { return b(off) | (b(off + 1) << 8); }
    __device__ __forceinline__ uint32_t r32(uint32_t off) const { return r16(off) | (r16(off + 2) << 16); }
    __device__ __forceinline__ void w8(uint32_t off, uint32_t v) { if (off < cap) p[off] = (uint8_t)v; }
    __device__ __forceinline__ void w16(uint32_t off, uint32_t v) { w8(off, v & 0xffu); w8(off + 1, (v >> 8) & 0xffu); }
    __device__ __forceinline__ void w32(uint32_t off, uint32_t v) { w16(off, v & 0xffffu); w16(off + 2, v >> 16); }
};

// Checksum arithmetic of bpf_l3_csum_replace / bpf_l4_csum_replace /
// bpf_csum_diff (Linux net/core/filter.c over include/net/checksum.h; the skb is
// a received frame, not CHECKSUM_PARTIAL).  Operands are raw LE loads of the
// network-order bytes, as the programs pass them.
#define GF_F_PSEUDO_HDR (1u << 4)
#define GF_F_MANGLED_0 (1u << 5)
__device__ __forceinline__ uint32_t ck_add(uint32_t a, uint32_t b) { uint32_t r = a + b; return r + (r < b ? 1u : 0u); }
__device__ __forceinline__ uint32_t ck_fold(uint32_t x) {
    x = (x & 0xffffu) + (x >> 16);
    x = (x & 0xffffu) + (x >> 16);
    return ~x & 0xffffu;
}
__device__ __forceinline__ uint32_t ck16_add(uint32_t a, uint32_t b) {
    uint32_t r = (a + b) & 0xffffu;
    return (r + (r < b ? 1u : 0u)) & 0xffffu;
}
// bpf_l3_csum_replace: size 0 = by diff, 2 = csum_replace2, 4 = csum_replace4
__device__ int l3_csum(Row &w, uint32_t len, int32_t off, uint32_t from, uint32_t to, uint32_t size) {
    if (!l4csum_ok(off, len)) return -GF_EFAULT;
    uint32_t sum = w.r16((uint32_t)off);
    if (size == 0) sum = ck_fold(ck_add(to, ~sum));
    else if (size == 2) sum = ~ck16_add(ck16_add(~sum & 0xffffu, ~from & 0xffffu), to & 0xffffu) & 0xffffu;
    else sum = ck_fold(ck_add(ck_add(~sum, ~from), to));
    w.w16((uint32_t)off, sum);
    return 0;
}
// bpf_l4_csum_replace (inet_proto_csum_replace4 / _by_diff, BPF_F_MARK_MANGLED_0)
__device__ int l4_csum(Row &w, uint32_t len, int32_t off, uint32_t from, uint32_t to, uint32_t flags) {
    if (!l4csum_ok(off, len)) return -GF_EFAULT;
    uint32_t sum = w.r16((uint32_t)off);
    const bool mmzero = (flags & GF_F_MANGLED_0) != 0;
    if (mmzero && !sum) return 0;
    if ((flags & 0xfu) == 0) sum = ck_fold(ck_add(to, ~sum));
    else sum = ck_fold(ck_add(ck_add(~sum, ~from), to));
    if (mmzero && !sum) sum = 0xffffu;                  // CSUM_MANGLED_0
    w.w16((uint32_t)off, sum);
    return 0;
}

// ================================================================ XDP
struct XdpDev {
    gf_htab_desc h4, h6, lxc;
    gf_trie_desc l4, l6;
    uint32_t has_h4, has_h6;
    // optional: the /32 map's and cilium_lxc's IPv4 keys as compact address sets
    // (Map::addr_set) probed in place of their hash tables (IPv4 only)
    const uint32_t *h4set, *lxset;
    uint32_t h4bits, lxbits, h4zero, lxzero;
    // optional (GF_XDP_DIR24, Map::dir24): the v4 prefixes as DIR-24-8 tables, read
    // in place of the trie walk below a root-summary "has a node" bit
    const uint16_t *d24;
    const uint32_t *d8;
};
// DIR-24-8 coverage of an IPv4 source (raw network-order word): one 2-B read of
// tbl24, one 4-B read of the /24's group when it holds longer prefixes.
__device__ __forceinline__ bool dir24_cov(const uint16_t *t24, const uint32_t *t8, uint32_t sa) {
    const uint32_t i24 = ((sa & 0xffu) << 16) | (sa & 0xff00u) | ((sa >> 16) & 0xffu), b = sa >> 24;
    const uint32_t e = gload<uint16_t>(t24 + i24);
    if (e == 0xffffu) return true;
    return e && ((gload<uint32_t>(t8 + (e - 1u) * 8u + (b >> 5)) >> (b & 31u)) & 1u);
}
// The table slot of an address in an endpoint-key set (its second array), or -1.
__device__ __forceinline__ int64_t aset_slot(const uint32_t *t, uint32_t bits, uint32_t zero, uint32_t a) {
    if (!a) return (int64_t)zero - 1;
    const uint32_t m = (1u << bits) - 1u;
    for (uint32_t k = gf_aset_home(a, bits);; k = (k + 1) & m) {
        const uint32_t v = t[k];
        if (v == a) return (int64_t)t[(1u << bits) + k];
        if (!v) return -1;
    }
}
// Membership in a compact IPv4 address set (gf_aset_home; <= 1/2 load), in LDS
// (k_xdp_lds) or in HBM / L2.
__device__ __forceinline__ bool aset_has(const uint32_t *t, uint32_t bits, uint32_t zero, uint32_t a) {
    if (!a) return zero != 0;
    const uint32_t m = (1u << bits) - 1u;
    for (uint32_t k = gf_aset_home(a, bits);; k = (k + 1) & m) {
        const uint32_t v = t[k];
        if (v == a) return true;
        if (!v) return false;
    }
}

__device__ __forceinline__ bool lxc_has4(const gf_htab_desc &lxc, uint32_t daddr) {
    uint32_t kw[5] = {daddr, 0, 0, 0, 1u};          // endpoint_key {ip4, pad.., family=1}
    return ht_find<20>(lxc, kw, key_hash<20>(kw)) >= 0;
}
__device__ __forceinline__ bool lxc_has6(const gf_htab_desc &lxc, const uint32_t *d) {
    uint32_t kw[5] = {d[0], d[1], d[2], d[3], 2u};
    return ht_find<20>(lxc, kw, key_hash<20>(kw)) >= 0;
}

// xdp_start -> check_filters -> check_v4 / check_v6 (bpf/bpf_xdp.c:97-184) for
// packet i; ab accumulates the algorithmic bytes.  The three lookups (the LPM
// trie, the /32 or /128 hash, the cilium_lxc endpoint) have no side effects, so
// the hash probes' home lines could be loaded before the trie walk (all in flight
// together).  Measured on config 1 (r2): 0.080 ms with both lines preloaded, 0.076
// with the prefix hash only, 0.075 with none — k_xdp is bound by the request rate
// of its L2-resident tables, not by the latency of the chain, so each probe is
// issued only when the reference would.
#define GF_XDP_U 2
template <class A>
__device__ __forceinline__ uint8_t xdp_verdict(const XdpDev &x, const A &a, uint32_t len, uint32_t et, uint32_t &ab) {
    if (len < 14) return XDP_DROP_;
    if (et == 0x0800) {
        if (len < 34) return XDP_DROP_;
        uint32_t sa = a.saddr4();
        const uint32_t kw[2] = {32u, sa};
        const uint32_t lk[5] = {a.daddr4(), 0, 0, 0, 1u};     // endpoint_key {ip4, pad.., family=1}
        ProbeLine<20, GF_XDP_U> ll;
        ProbeLine<8, GF_XDP_U> hl;
        bool drop = false;
        ab += 10;
        if (x.has_h4) {
            ab += 9;
            bool cov;
            if (x.l4.rsum) {                            // the root summary: covered / has a node / neither
                const uint32_t idx = ((sa & 0xffu) << 8) | ((sa >> 8) & 0xffu);
                cov = (gload<uint64_t>(x.l4.rsum + (idx >> 6)) >> (idx & 63)) & 1ull;
                if (!cov && ((gload<uint64_t>(x.l4.rsum + 1024 + (idx >> 6)) >> (idx & 63)) & 1ull))
                    cov = x.d24 ? dir24_cov(x.d24, x.d8, sa)
                                : trie_nodes<1>(x.l4, AddrBytes<1>(&sa), gload<uint32_t>(x.l4.root + idx) - 1u);
            } else {
                cov = trie_lookup<1>(x.l4, &sa);
            }
            if (cov) drop = true;
            else {
                ab += 9;
                if (x.h4set) drop = aset_has(x.h4set, x.h4bits, x.h4zero, sa);
                else {
                    hl.load(x.h4, key_hash<8>(kw));
                    drop = probe2<8, GF_XDP_U, 0>(x.h4, kw, kw, hl, false).f >= 0;
                }
            }
        }
        if (drop) return XDP_DROP_;
        ab += 20;
        if (x.lxset) return aset_has(x.lxset, x.lxbits, x.lxzero, lk[0]) ? XDP_PASS_ : XDP_DROP_;
        ll.load(x.lxc, key_hash<20>(lk));
        return probe2<20, GF_XDP_U, 0>(x.lxc, lk, lk, ll, false).f >= 0 ? XDP_PASS_ : XDP_DROP_;
    }
    if (et == 0x86DD) {
        if (len < 54 || !a.has6()) return XDP_DROP_;
        uint4 s = a.saddr6();
        uint32_t sw[4] = {s.x, s.y, s.z, s.w};
        const uint32_t kw[5] = {128u, s.x, s.y, s.z, s.w};
        const uint4 d = a.daddr6();
        const uint32_t lk[5] = {d.x, d.y, d.z, d.w, 2u};
        ProbeLine<20, GF_XDP_U> ll;
        ProbeLine<20, GF_XDP_U> hl;
        bool drop = false;
        ab += 34;
        if (x.has_h6) {
            ab += 21;
            if (trie_lookup<4>(x.l6, sw)) drop = true;
            else {
                ab += 21;
                hl.load(x.h6, key_hash<20>(kw));
                drop = probe2<20, GF_XDP_U, 0>(x.h6, kw, kw, hl, false).f >= 0;
            }
        }
        if (drop) return XDP_DROP_;
        ab += 20;
        ll.load(x.lxc, key_hash<20>(lk));
        return probe2<20, GF_XDP_U, 0>(x.lxc, lk, lk, ll, false).f >= 0 ? XDP_PASS_ : XDP_DROP_;
    }
    return XDP_PASS_;
}

__global__ __launch_bounds__(BLOCK) void k_xdp(gf_pkt_cols c, XdpDev x, uint8_t *verdict,
                                               unsigned long long *stats) {
    __shared__ uint32_t sl[272];
    Stats st{sl};
    if (stats) st.init();
    uint32_t n_drop = 0, n_pass = 0, s_len = 0, s_ab = 0;      // the lane's counter sums (Stats::xdp_sums)
    for (uint32_t b = blockIdx.x * blockDim.x; b < c.n; b += gridDim.x * blockDim.x) {
        const uint32_t i = b + threadIdx.x;
        if (i < c.n) {
            uint32_t ab = 1;                               // output record
            const uint32_t len = c.len[i];
            const uint8_t v = xdp_verdict(x, ColA{c, i}, len, c.ethertype[i], ab);
            verdict[i] = v;
            n_drop += v == XDP_DROP_; n_pass += v == XDP_PASS_; s_len += len; s_ab += ab;
        }
    }
    if (stats) { st.xdp_sums(n_drop, n_pass, s_len, s_ab); st.flush(stats); }
}

// check_v4 with the prefilter's hot levels in LDS (k_xdp_lds): the trie's
// 2^16-entry root as two bitmaps (covered: drop at once / has a node: walk on in
// HBM), and — when they fit — the /32 hash's slot array and cilium_lxc's key
// slots, staged once per block (one or two 1024-lane blocks per CU, grid-stride
// over the batch).  The lookups and their order are xdp_verdict's; IPv6 and
// other frames take xdp_verdict as it is.
struct XdpLds {
    uint32_t h4_bytes, lxc_bytes;                  // slot arrays staged as they are (0: not staged)
    const uint32_t *h4set, *lxset;                 // or the tables' compact address sets (Map::addr_set)
    uint32_t h4bits, lxbits, h4zero, lxzero;
};

// Exact-match probe over a slot array held in LDS (layout as in HBM).
template <int KSZ>
__device__ __forceinline__ bool lds_has(const uint8_t *slots, uint64_t mask, uint32_t slot_size, const uint32_t *kw,
                                        uint32_t h) {
    constexpr int SW = KSZ / 4;
    static_assert(KSZ % 4 == 0, "word keys");
    const uint32_t m = (uint32_t)mask, i = (uint32_t)gf_home_slot(h, mask, slot_size);   // LDS tables: < 2^32 slots
    for (uint32_t p = 0; p <= m; p++) {
        const uint32_t *w = reinterpret_cast<const uint32_t *>(slots + ((i + p) & m) * slot_size);
        const uint32_t st = w[SW] & 0xffu;
        if (st == GF_SLOT_EMPTY) return false;
        if (st == GF_SLOT_FULL) {
            bool e = true;
#pragma unroll
            for (int k = 0; k < SW; k++) e &= w[k] == kw[k];
            if (e) return true;
        }
    }
    return false;
}
__global__ __launch_bounds__(1024) void k_xdp_lds(gf_pkt_cols c, XdpDev x, XdpLds L, uint8_t *verdict,
                                                  unsigned long long *stats) {
    extern __shared__ uint4 xl[];
    __shared__ uint32_t sl[272];
    Stats st{sl};
    const uint64_t *rs = reinterpret_cast<const uint64_t *>(xl);
    const uint32_t h4b = L.h4set ? 4u << L.h4bits : L.h4_bytes, lxb = L.lxset ? 4u << L.lxbits : L.lxc_bytes;
    const uint8_t *h4s = reinterpret_cast<const uint8_t *>(xl) + GF_TRIE_RSUM_BYTES;
    const uint8_t *lxs = h4s + h4b;
    {
        uint4 *d = xl;
        const uint4 *src = reinterpret_cast<const uint4 *>(x.l4.rsum);
        for (uint32_t k = threadIdx.x; k < GF_TRIE_RSUM_BYTES / 16; k += blockDim.x) d[k] = src[k];
        d += GF_TRIE_RSUM_BYTES / 16;
        src = reinterpret_cast<const uint4 *>(L.h4set ? (const void *)L.h4set : (const void *)x.h4.slots);
        for (uint32_t k = threadIdx.x; k < h4b / 16; k += blockDim.x) d[k] = src[k];
        d += h4b / 16;
        src = reinterpret_cast<const uint4 *>(L.lxset ? (const void *)L.lxset : (const void *)x.lxc.slots);
        for (uint32_t k = threadIdx.x; k < lxb / 16; k += blockDim.x) d[k] = src[k];
    }
    if (stats) st.init(); else __syncthreads();
    uint32_t n_drop = 0, n_pass = 0, s_len = 0, s_ab = 0;      // the lane's counter sums, reduced once at the end
    for (uint32_t b = blockIdx.x * blockDim.x; b < c.n; b += gridDim.x * blockDim.x) {   // wave-uniform trips
        const uint32_t i = b + threadIdx.x;
        const bool act = i < c.n;
        uint32_t len = 0, ab = 1;
        uint8_t v = 0;
        if (act) {
            len = c.len[i];
            const uint32_t et = c.ethertype[i];
            if (et != 0x0800 || len < 34) {
                v = xdp_verdict(x, ColA{c, i}, len, et, ab);
            } else {
                const uint32_t sa = c.saddr4[i];
                bool drop = false;
                ab += 10;
                if (x.has_h4) {
                    ab += 9;
                    const uint32_t idx = ((sa & 0xffu) << 8) | ((sa >> 8) & 0xffu);   // the first two address bytes
                    if ((rs[idx >> 6] >> (idx & 63)) & 1ull) drop = true;
                    else if ((rs[1024 + (idx >> 6)] >> (idx & 63)) & 1ull)
                        drop = x.d24 ? dir24_cov(x.d24, x.d8, sa)
                                     : trie_nodes<1>(x.l4, AddrBytes<1>(&sa), gload<uint32_t>(x.l4.root + idx) - 1u);
                    if (!drop) {
                        ab += 9;
                        const uint32_t kw[2] = {32u, sa};
                        drop = L.h4set ? aset_has(reinterpret_cast<const uint32_t *>(h4s), L.h4bits, L.h4zero, sa)
                             : L.h4_bytes ? lds_has<8>(h4s, x.h4.mask, x.h4.slot_size, kw, key_hash<8>(kw))
                                          : ht_find<8>(x.h4, kw, key_hash<8>(kw)) >= 0;
                    }
                }
                if (drop) {
                    v = XDP_DROP_;
                } else {
                    ab += 20;
                    const uint32_t lk[5] = {c.daddr4[i], 0, 0, 0, 1u};
                    const bool ep = L.lxset ? aset_has(reinterpret_cast<const uint32_t *>(lxs), L.lxbits, L.lxzero, lk[0])
                                  : L.lxc_bytes ? lds_has<20>(lxs, x.lxc.mask, x.lxc.slot_size, lk, key_hash<20>(lk))
                                                : ht_find<20>(x.lxc, lk, key_hash<20>(lk)) >= 0;
                    v = ep ? XDP_PASS_ : XDP_DROP_;
                }
            }
            verdict[i] = v;
            n_drop += v == XDP_DROP_; n_pass += v == XDP_PASS_; s_len += len; s_ab += ab;
        }
    }
    if (stats) {
        st.xdp_sums(n_drop, n_pass, s_len, s_ab);
        st.flush(stats);
    }
}

// ================================================================ LB
struct LbDev {
    gf_htab_desc s4, s6;
    uint32_t flags;
};

__device__ __forceinline__ int lb_checks(const LbDev &L, uint32_t len, int l4_off, uint32_t nh,
                                         uint32_t key_dport, uint32_t svc_port, bool v6, uint16_t *new_dport) {
    uint32_t co = csum_l4_offset(nh);
    if ((co || v6) && !l4csum_ok(l4_off + (int)co, len)) return D_CSUM_L4;
    if ((L.flags & GF_LB_F_L4) && svc_port && key_dport != svc_port && (nh == 6 || nh == 17)) {
        if (!l4csum_ok(l4_off + (int)co, len)) return D_CSUM_L4;
        if (!skb_ok(l4_off + 2, 2, len)) return D_WRITE_ERROR;
        *new_dport = (uint16_t)svc_port;
    }
    return TC_OK;
}

// returns program result (TC_OK pass / TC_REDIRECT translated / negative error)
template <class A>
__device__ int lb_v4(const LbDev &L, const A &a, uint32_t len, gf_lb_out &o, uint32_t &ab, uint32_t &key_dport) {
    if (len < 34) return D_INVALID;
    uint32_t nh = a.proto(), daddr = a.daddr4();
    int l4_off = a.l4_off();
    uint32_t dport = 0;
    if (L.flags & GF_LB_F_L4) {
        if (nh == 6 || nh == 17) {
            if (!skb_ok(l4_off + 2, 2, len)) return -GF_EFAULT;
            dport = a.l4w0() >> 16;
        } else if (nh != 1 && nh != 58) return TC_OK;     // DROP_UNKNOWN_L4 -> pass
    }
    const uint8_t *svc = nullptr;
    if ((L.flags & GF_LB_F_L4) && dport) {
        uint32_t kw[2] = {daddr, dport};
        int64_t f = ht_find<8>(L.s4, kw, key_hash<8>(kw));
        ab += 20;
        if (f >= 0) { const uint8_t *v = ht_val(L.s4, f); if (gload<uint16_t>(v + 6)) svc = v; }
        if (!svc) dport = 0;
    }
    if (!svc && (L.flags & GF_LB_F_L3)) {
        uint32_t kw[2] = {daddr, dport};
        int64_t f = ht_find<8>(L.s4, kw, key_hash<8>(kw));
        ab += 20;
        if (f >= 0) { const uint8_t *v = ht_val(L.s4, f); if (gload<uint16_t>(v + 6)) svc = v; }
    }
    if (!svc) return TC_OK;
    uint32_t count = gload<uint16_t>(svc + 6);
    uint32_t slave = (a.fhash() % count + 1u) & 0xffffu;
    uint32_t kw[2] = {daddr, dport | (slave << 16)};
    int64_t f = ht_find<8>(L.s4, kw, key_hash<8>(kw));
    ab += 20;
    if (f < 0) return D_NO_SERVICE;
    const uint8_t *be = ht_val(L.s4, f);
    uint32_t target = gload<uint32_t>(be);
    uint32_t port = gload<uint16_t>(be + 4);
    uint32_t rn = gload<uint16_t>(be + 8);
    uint16_t nd = 0;
    int r = lb_checks(L, len, l4_off, nh, dport, port, false, &nd);
    if (r < 0) return r;
    key_dport = dport;
    o.slave = (uint16_t)slave; o.new_dport = nd; o.rev_nat = (uint16_t)rn; o.new_daddr4 = target;
    return TC_REDIRECT;
}

template <class A>
__device__ int lb_v6(const LbDev &L, const A &a, uint32_t len, gf_lb_out &o, uint32_t *nd6, uint32_t &ab,
                     uint32_t &key_dport) {
    if (len < 54 || !a.has6()) return D_INVALID;
    uint32_t nh = a.proto();
    int l4_off = a.l4_off();
    uint4 d = a.daddr6();
    uint32_t dport = 0;
    if (L.flags & GF_LB_F_L4) {
        if (nh == 6 || nh == 17) {
            if (!skb_ok(l4_off + 2, 2, len)) return -GF_EFAULT;
            dport = a.l4w0() >> 16;
        } else if (nh != 1 && nh != 58) return TC_OK;
    }
    const uint8_t *svc = nullptr;
    if ((L.flags & GF_LB_F_L4) && dport) {
        uint32_t kw[5] = {d.x, d.y, d.z, d.w, dport};
        int64_t f = ht_find<20>(L.s6, kw, key_hash<20>(kw));
        ab += 44;
        if (f >= 0) { const uint8_t *v = ht_val(L.s6, f); if (gload<uint16_t>(v + 18)) svc = v; }
        if (!svc) dport = 0;
    }
    if (!svc && (L.flags & GF_LB_F_L3)) {
        uint32_t kw[5] = {d.x, d.y, d.z, d.w, dport};
        int64_t f = ht_find<20>(L.s6, kw, key_hash<20>(kw));
        ab += 44;
        if (f >= 0) { const uint8_t *v = ht_val(L.s6, f); if (gload<uint16_t>(v + 18)) svc = v; }
    }
    if (!svc) return TC_OK;
    uint32_t count = gload<uint16_t>(svc + 18);
    uint32_t slave = (a.fhash() % count + 1u) & 0xffffu;
    uint32_t kw[5] = {d.x, d.y, d.z, d.w, dport | (slave << 16)};
    int64_t f = ht_find<20>(L.s6, kw, key_hash<20>(kw));
    ab += 44;
    if (f < 0) return D_NO_SERVICE;
    const uint8_t *be = ht_val(L.s6, f);
    uint32_t t[4];
    for (int k = 0; k < 4; k++) t[k] = gload<uint32_t>(be + 4 * k);
    uint32_t port = gload<uint16_t>(be + 16);
    uint32_t rn = gload<uint16_t>(be + 20);
    if (rn) t[3] |= rn;
    uint16_t ndp = 0;
    int r = lb_checks(L, len, l4_off, nh, dport, port, true, &ndp);
    if (r < 0) return r;
    key_dport = dport;
    o.slave = (uint16_t)slave; o.new_dport = ndp; o.rev_nat = (uint16_t)rn;
    for (int k = 0; k < 4; k++) nd6[k] = t[k];
    return TC_REDIRECT;
}

__global__ __launch_bounds__(BLOCK) void k_lb(gf_pkt_cols c, LbDev L, gf_lb_out *out, uint8_t *nd6,
                                              unsigned long long *stats) {
    __shared__ uint32_t sl[272];
    Stats st{sl};
    if (stats) st.init();
    uint32_t s_n = 0, s_len = 0, s_ab = 0;              // the lane's packet count and sums (Stats::sums)
    // wave-uniform trip count (the stats aggregation is a wave collective)
    for (uint32_t b = blockIdx.x * blockDim.x; b < c.n; b += gridDim.x * blockDim.x) {
      const uint32_t i = b + threadIdx.x;
      const bool act = i < c.n;
      gf_lb_out o{};
      uint32_t len = 0;
      uint32_t ab = 12 + 12;                              // header columns + output record
      if (act) {
        uint32_t n6[4] = {0, 0, 0, 0};
        len = c.len[i];
        const uint32_t et = c.ethertype[i];
        int ret = TC_OK;
        bool v6 = false;
        uint32_t kd = 0;
        if (et == 0x86DD) { if (!(L.flags & GF_LB_F_NO_IPV6)) { v6 = true; ab += 28; ret = lb_v6(L, ColA{c, i}, len, o, n6, ab, kd); } }
        else if (et == 0x0800) { if (!(L.flags & GF_LB_F_NO_IPV4)) ret = lb_v4(L, ColA{c, i}, len, o, ab, kd); }
        if (ret < 0 || ret == TC_SHOT) {
            o = gf_lb_out{};
            o.action = TC_SHOT; o.reason = (uint8_t)(-ret);
            n6[0] = n6[1] = n6[2] = n6[3] = 0;
        } else {
            o.action = ((L.flags & GF_LB_F_REDIRECT) && ret == TC_REDIRECT) ? TC_REDIRECT : TC_OK;
        }
        out[i] = o;
        if (nd6 && v6) reinterpret_cast<uint4 *>(nd6)[i] = make_uint4(n6[0], n6[1], n6[2], n6[3]);
        else if (nd6) reinterpret_cast<uint4 *>(nd6)[i] = make_uint4(0, 0, 0, 0);
      }
      if (act) { s_n++; s_len += len; s_ab += ab; }
      if (stats) st.bins_wave(act, o.reason, o.action);
    }
    if (stats) { st.sums(s_n, s_len, s_ab); st.flush(stats); }
}

// ================================================================ ingress (handle_policy)
// Device-only program flags (high bits of gf_lxc_dev.flags): the program binds
// the CT map of that family (all programs share one per family, X.ct4 / X.ct6).
#define GF_LXC_DEV_HAS_CT4 (1u << 30)
#define GF_LXC_DEV_HAS_CT6 (1u << 31)

// The ICMP-related entries of an egress connection-group run: the
// only CT keys two connections of one address pair share, written (BPF_ANY) by every
// new connection of the pair in both passes and read by nothing in the run.  Only the
// last write of each key in batch order survives, so each write enters its key here
// instead of a log: the key {daddr, saddr} of the related tuple (its ports are 0 and
// its flags byte is 2 | direction, which picks one of the slot's two words) claims a
// slot (open addressing, 0 = empty; key 0 has the extra slot mask + 1), and the word
// keeps 1 + the highest order written (2i: packet i's from-container create, 2i + 1:
// its delivery's).  k_rset_apply rebuilds each winner's value from its packet.
struct RelSet {
    unsigned long long *slot;          // mask + 2 slots of 16 B: the key, then its two words
    uint32_t *list, *list_n;           // the claimed slots, for the apply
    uint32_t mask;
};
struct IngCtx {
    const gf_lxc_dev *cfgs;
    const uint8_t *saddr6, *daddr6;
    uint32_t a6_stride;      // bytes between two packets' v6 addresses: 16 (the caller's columns) or 32 (the
                             // pipeline / egress deliveries: both addresses of a packet in one 32-B piece)
    gf_htab_desc ct4, ct6;   // cilium_ct4_global / cilium_ct6_global (shared by every program)
    uint32_t now, host_ifindex;
    uint32_t strict;   // bit0 / bit1: CT4 / CT6 inserts check max_entries with atomics
    uint8_t *pout;     // pipeline records (gf_pipeline_out) to complete instead of gf_ingress_out
    uint32_t pout_wo;  // gf_pipeline_classify: the record's first 10 bytes are written without reading them
    uint32_t pol_wave; // policy counter adds summed per wave first (pol_count_add): the egress deliveries' pass
                       // (stage POLICY, the front's GF_PIPE_F_* bits 5-7 in gf_rec.cls bits 4-6)
    uint8_t *snap;     // pipeline: the frames as rewritten so far (handle_policy's writes land here)
    uint32_t snap_stride;
    uint32_t *plog, *plog_n;   // cilium_proxy{4,6} update log (16 words per redirect) and its length
    uint32_t gw, host6[4];     // IPV4_GATEWAY, HOST_IP (node_config.h)
    uint8_t *tmark, *tcap;     // trace notifications: per-packet GF_TR_* marks, 128-B captures (null: off)
    uint32_t *rlog, *rlog_n;   // egress connection groups: ct_create4's related entries logged (null: written)
    const uint32_t *rlog_off;  // device word: nonzero = the run fell back to pair groups (entries written inline)
    RelSet rs;                 // the related entries' set (rlog non-null: in use; slot null: the log itself)
};

// ---- handle_policy's own header writes (kept out of line: cold paths of the
// hot kernel) and the proxy-map log ----
// The IngCtx fields the writers read, passed by value to the out-of-line copies:
// a reference (or a pointer to a local tuple) would keep the whole context (or
// the tuple) in scratch for the entire IPv6 kernel.
struct PolCtx {
    uint8_t *snap;
    uint32_t *plog, *plog_n;
    uint32_t snap_stride, now, gw, host6[4];
};
__device__ __forceinline__ PolCtx pol_ctx(const IngCtx &X) {
    PolCtx c;
    c.snap = X.snap; c.plog = X.plog; c.plog_n = X.plog_n;
    c.snap_stride = X.snap_stride; c.now = X.now; c.gw = X.gw;
    for (int k = 0; k < 4; k++) c.host6[k] = X.host6[k];
    return c;
}
template <class XC>
__device__ __forceinline__ Row pol_row(const XC &X, uint32_t i, uint32_t len) {
    return Row{X.snap + (size_t)i * X.snap_stride, X.snap_stride < len ? X.snap_stride : len};
}
// Trace notifications (bpf/lib/trace.h:59-106).  The records themselves are
// written after the launches by the event pass (k_ev_*), from the verdict
// records; the kernels only leave what the records cannot tell: a per-packet
// mark byte and, for TRACE_TO_PROXY, the frame as it was when the redirect sent
// it (before its own rewrites, lib/lxc.h:115-117 / 167-169).
#define GF_TR_PX_EGRESS 1u    // from-container ipv{4,6}_redirect_to_host_port entered (TRACE_TO_PROXY)
#define GF_TR_PX_POLICY 2u    // handle_policy's ipv{4,6}_redirect_to_host_port entered (TRACE_TO_PROXY)
#define GF_TR_CLUSTER   4u    // from-container dstID == CLUSTER_ID (TRACE_TO_STACK's dst_label)
#define GF_TR_CAPTURED 16u    // tcap holds the TO_PROXY capture
// f: the frame in HBM; a/na: header bytes a kernel holds in an LDS copy (they
// replace the frame's first na bytes); cap = min(len, stride, TRACE_PAYLOAD_LEN).
__device__ __forceinline__ void trace_proxy(uint8_t *tmark, uint8_t *tcap, const uint8_t *f, const uint8_t *a,
                                            uint32_t na, uint32_t cap, uint32_t i, uint32_t bit) {
    uint32_t m = tmark[i] | bit;
    if (f) {
        uint8_t *d = tcap + (size_t)i * GF_TRACE_PAYLOAD_LEN;
        for (uint32_t k = 0; k < GF_TRACE_PAYLOAD_LEN; k += 4) {
            uint32_t v = 0;
            for (uint32_t b = 0; b < 4; b++) {
                const uint32_t o = k + b;
                if (o < cap) v |= (uint32_t)(o < na ? a[o] : f[o]) << (8 * b);
            }
            *reinterpret_cast<uint32_t *>(d + k) = v;
        }
        m |= GF_TR_CAPTURED;
    }
    tmark[i] = (uint8_t)m;
}
__device__ __forceinline__ uint32_t trace_cap_len(uint32_t len, uint32_t stride) {
    const uint32_t c = len < stride ? len : stride;
    return c < GF_TRACE_PAYLOAD_LEN ? c : GF_TRACE_PAYLOAD_LEN;
}
// reverse_map_l4_port (bpf/lib/lb.h:217-251) + __lb4_rev_nat / __lb6_rev_nat
// (lb.h:253-293, 447-512; v4 with REV_NAT_F_TUPLE_SADDR: the old address is the
// tuple's, v6 with flags 0: the frame's)
template <class XC>
__device__ __forceinline__ void pol_rev_nat_write(const XC &X, uint32_t i, uint32_t len, int l4_off,
                                                            uint32_t nh, const uint8_t *nat, bool v6,
                                                            uint32_t old_sip4) {
    Row w = pol_row(X, i, len);
    const uint32_t co = csum_l4_offset(nh), fl = nh == 17 ? GF_F_MANGLED_0 : 0u;
    const uint32_t port = gload<uint16_t>(nat + (v6 ? 16 : 4));
    if (port && (nh == 6 || nh == 17)) {
        const uint32_t old = w.r16((uint32_t)l4_off);
        if (port != old) {
            l4_csum(w, len, l4_off + (int)co, old, port, 2u | fl);
            w.w16((uint32_t)l4_off, port);
        }
    }
    uint32_t sum = 0;
    if (!v6) {
        const uint32_t nw = gload<uint32_t>(nat);
        w.w32(26, nw);
        sum = ck_add(ck_add(0u, ~old_sip4), nw);
        l3_csum(w, len, 24, 0, sum, 0);
        if (co) l4_csum(w, len, l4_off + (int)co, 0, sum, GF_F_PSEUDO_HDR | fl);
    } else {
        for (int k = 0; k < 4; k++) {
            const uint32_t od = w.r32(22 + 4 * k), nw = gload<uint32_t>(nat + 4 * k);
            w.w32(22 + 4 * k, nw);
            sum = ck_add(ck_add(sum, ~od), nw);
        }
        l4_csum(w, len, l4_off + (int)co, 0, sum, GF_F_PSEUDO_HDR | fl);
    }
}
// ipv6_policy's "derive reverse NAT index and zero it" (bpf_lxc.c:774-790)
template <class XC>
__device__ __forceinline__ void pol_v6_zero_rn(const XC &X, uint32_t i, uint32_t len, int l4_off,
                                                         uint32_t nh, uint32_t rn) {
    Row w = pol_row(X, i, len);
    w.w16(38 + 12, 0);
    const uint32_t co = csum_l4_offset(nh);
    if (co) l4_csum(w, len, l4_off + (int)co, 0, ck_add(ck_add(0u, ~rn), 0u),
                    GF_F_PSEUDO_HDR | (nh == 17 ? GF_F_MANGLED_0 : 0u));
}
// ipv{4,6}_redirect_to_host_port writes (lib/lxc.h:96-205) after their checks,
// and the cilium_proxy{4,6} entry, logged for the in-order apply after the launch.
// t: the CT tuple words as ct_lookup left them; od: the original daddr.
template <class XC>
__device__ __forceinline__ void pol_redirect(const XC &X, uint32_t i, uint32_t len, int l4_off,
                                                       uint32_t nh, const uint32_t *t, bool v6, uint32_t new_port,
                                                       const uint32_t *od, uint32_t identity, uint32_t egress = 0) {
    const uint32_t pw = v6 ? t[8] : t[2];
    const uint32_t old_port = pw & 0xffffu, sport = pw >> 16;
    if (X.snap) {
        Row w = pol_row(X, i, len);
        const uint32_t co = csum_l4_offset(nh), fl = nh == 17 ? GF_F_MANGLED_0 : 0u;
        l4_csum(w, len, l4_off + (int)co, old_port, new_port, 2u | fl);     // l4_modify_port
        w.w16((uint32_t)(l4_off + 2), new_port);
        if (!v6) {
            w.w32(30, X.gw);
            l3_csum(w, len, 24, od[0], X.gw, 4);
            if (co) l4_csum(w, len, l4_off + (int)co, od[0], X.gw, 4u | GF_F_PSEUDO_HDR | fl);
        } else {
            uint32_t sum = 0;
            for (int k = 0; k < 4; k++) {
                w.w32(38 + 4 * k, X.host6[k]);
                sum = ck_add(ck_add(sum, ~od[k]), X.host6[k]);
            }
            if (co) l4_csum(w, len, l4_off + (int)co, 0, sum, GF_F_PSEUDO_HDR | fl);
        }
    }
    if (X.plog) {
        uint32_t *e = X.plog + 16ull * atomicAdd(X.plog_n, 1u);
        uint32_t q[16] = {0};
        q[0] = i; q[1] = v6 ? 6u : 4u;
        const int a = v6 ? 4 : 1;                       // key: .saddr = tuple->daddr, .dport, .sport, .nexthdr
        for (int k = 0; k < a; k++) q[2 + k] = t[k];
        q[2 + a] = new_port | (sport << 16);
        q[3 + a] = nh;
        for (int k = 0; k < a; k++) q[8 + k] = od[k];  // value: orig_daddr, orig_dport, identity, lifetime
        q[8 + a] = old_port;
        q[9 + a] = identity;
        q[10 + a] = X.now + 720u;                       // PROXY_DEFAULT_LIFETIME
        q[15] = egress;                                 // from-container entry: no handle_policy MAC stores
        for (int k = 0; k < 16; k += 4) *reinterpret_cast<uint4 *>(e + k) = make_uint4(q[k], q[k + 1], q[k + 2], q[k + 3]);
    }
}

struct CtState { uint32_t rev_nat, loopback, carry; };

// Slot headers fetched per probe step.  CT maps use the hot-split layout
// (gf_common.h): CT4 slots are 32 B (2 per step = one 64-B request), CT6 64 B;
// policy maps the 16-B policy layout (4 per step = one 64-B request).
// Results do not depend on these.
#ifndef GF_CT4_U
#define GF_CT4_U 2
#endif
#define GF_CT6_U 1
#ifndef GF_POL_U
#define GF_POL_U 4
#endif
#define GF_POL_SLOT 16u    // policy layout (GF_VCODEC_POL, gf_common.h): key | state | pad | proxy_port
#define GF_POL_VOFF 10u
#define GF_POL_SIDE 24u    // side array: packets, bytes, pad

// The endpoint program of the lane's current packet, kept in registers while
// consecutive packets of the lane's bucket target the same endpoint.
struct Ep {
    uint32_t sl;                     // program slot + 1 (0: none loaded)
    uint32_t flags;
    uint8_t *pol;                    // policy map slots / side array / mask (< 2^32 slots)
    uint8_t *pol_side;
    uint32_t pol_mask;
    uint32_t next;                   // round-robin bits: bit0 counter sums (PolAcc), bit1 decisions (PolMemo)
    __device__ __forceinline__ void init() { sl = 0; flags = 0; pol = pol_side = nullptr; pol_mask = 0; next = 0; }
    __device__ __forceinline__ void use(const IngCtx &X, uint32_t s) {
        if (s == sl) return;
        sl = s;
        const gf_lxc_dev *c = X.cfgs + (s - 1);
        flags = gload<uint32_t>(&c->flags);
        pol = gload<uint8_t *>(&c->policy.slots);
        pol_side = gload<uint8_t *>(&c->policy.vals);
        pol_mask = (uint32_t)gload<uint64_t>(&c->policy.mask);
    }
    __device__ __forceinline__ const gf_lxc_dev *cfg(const IngCtx &X) const { return X.cfgs + (sl - 1); }
    __device__ __forceinline__ gf_htab_desc pdesc() const {
        gf_htab_desc d{};
        d.slots = pol; d.vals = pol_side; d.mask = pol_mask; d.ksz = 8; d.vsz = 24;
        d.slot_size = GF_POL_SLOT; d.voff = GF_POL_VOFF; d.vin = 2; d.split = 1; d.sstride = GF_POL_SIDE;
        return d;
    }
};

// The CT map a packet's program binds (CT_MAP4 / CT_MAP6 of its endpoint).
// PCT = false: every program binds the global map (cilium_ct4_global /
// cilium_ct6_global), passed once in the launch context.  PCT = true: the
// ConntrackLocal layout (pkg/endpoint/bpf.go:268-276, cilium_ct4_<id>): each
// program's own map, read from the program table per packet.
template <int FAM, bool PCT>
__device__ __forceinline__ gf_htab_desc ing_ct(const IngCtx &X, const Ep &ep) {
    constexpr uint32_t has = FAM == 6 ? GF_LXC_DEV_HAS_CT6 : GF_LXC_DEV_HAS_CT4;
    if (!(ep.flags & has)) return gf_htab_desc{};
    if constexpr (PCT) return gload<gf_htab_desc>(FAM == 6 ? &ep.cfg(X)->ct6 : &ep.cfg(X)->ct4);
    else return FAM == 6 ? X.ct6 : X.ct4;
}

// The ICMP-related entry ct_create writes for every new flow of a group
// (conntrack.h:563-577) is the same key for the whole group: a lane keeps
// where it lives.  Only this lane changes keys of its group; a delete by the
// lane clears the cache.
// IPv4: the lane also keeps the entry's last hot-part rewrite
// pending instead of storing each one — the value of an ingress create's related
// entry is fixed by now (per launch), the protocol's timeout and the packet's
// length — in the spare high bits of the cached key's last word (bits 16-31: the
// length, bit 15: TCP), and writes it once: before a packet that could read it (an
// ICMP packet of the lane: only ct_lookup4's related probe matches the key),
// before the cache moves to another entry and at the end of the launch.  A group
// creating 4 flows a step then writes its related entry once instead of 4 times.
template <int TW>
struct RelCache {
    uint32_t k[TW];
    uint32_t slot;           // ~0u: none (tables of >= 2^32 slots are not cached)
    uint32_t sec;            // src_sec_id of the cold value part this lane wrote there
    __device__ __forceinline__ void init() { slot = ~0u; sec = 0; k[TW - 1] = 0; }
};
// The pending hot-part write of the IPv4 related entry (RelCache<4>::k[3] >> 15), if any.
__device__ __forceinline__ void rel_flush4(const gf_htab_desc &d, RelCache<4> &rc, uint32_t now) {
    const uint32_t p = rc.k[3] >> 15;
    if (!p) return;
    rc.k[3] &= 0x7fffu;
    if (rc.slot == ~0u || !d.slots) return;
    const uint32_t v[4] = {now + ((p & 1u) ? 300u : 43200u), F_SEEN_NON_SYN, 1u, p >> 1};
    store_words<4>(d.slots + (uint64_t)rc.slot * d.slot_size + d.voff, v);
    GF_WR(WR_REL_HOT);
}
template <int TW>
__device__ __forceinline__ void rel_drop(const gf_htab_desc &d, RelCache<TW> &rc, uint32_t now) {
    if constexpr (TW == 4) rel_flush4(d, rc, now);
    rc.slot = ~0u;
}

// __ct_lookup, bpf/lib/conntrack.h:75-135 (dir = CT_INGRESS), hit part.  CT
// values use the GF_VCODEC_CT layout: `hot` = the entry's first 16 B
// (lifetime, flags | rev_nat_index, rx_packets lo32, rx_bytes lo32), loaded
// with the key; the update is one 16-B store into the key's sector (the high
// halves of the rx counters are touched only on a 32-bit carry).
__device__ __forceinline__ void ct_hit(const gf_htab_desc &d, int64_t f, uint4 hot, int action, bool syn,
                                       uint32_t len, uint32_t now, bool acct, CtState &st, uint32_t &ab) {
    ab += 96;                                           // entry RMW: 48 B read + 48 B written
    uint8_t *e = ht_val(d, (uint64_t)f);
    uint32_t life = hot.x, fl = hot.y & 0xffffu, rn = hot.y >> 16;
    if (!(fl & F_RX_CLOSING) || !(fl & F_TX_CLOSING)) {  // ct_entry_alive -> ct_update_timeout
        if (!syn) fl |= F_SEEN_NON_SYN;
        life = now + ((fl & F_SEEN_NON_SYN) ? 43200u : 300u);
    }
    st.rev_nat = rn;
    st.loopback = (fl >> 3) & 1u;
    if (acct) {                                         // rx_packets += 1, rx_bytes += len (exclusive lane)
        uint32_t pk = hot.z + 1u, by = hot.w + len;
        uint8_t *hi = d.sstride ? ht_side(d, (uint64_t)f) : e + 16;
        if (pk == 0u) { gstore<uint32_t>(hi, gload<uint32_t>(hi) + 1u); st.carry = 1; GF_WR(WR_CARRY); }
        if (by < hot.w) { gstore<uint32_t>(hi + 4, gload<uint32_t>(hi + 4) + 1u); st.carry = 1; GF_WR(WR_CARRY); }
        hot.z = pk; hot.w = by;
    }
    if (action == ACT_CREATE) {
        if (fl & (F_RX_CLOSING | F_TX_CLOSING)) {
            fl &= ~(F_RX_CLOSING | F_TX_CLOSING);
            if (!syn) fl |= F_SEEN_NON_SYN;
            life = now + ((fl & F_SEEN_NON_SYN) ? 43200u : 300u);
        }
    } else if (action == ACT_CLOSE) {
        fl |= F_RX_CLOSING;
        if ((fl & F_RX_CLOSING) && (fl & F_TX_CLOSING)) life = now + 10u;
    }
    hot.x = life;
    hot.y = (hot.y & 0xffff0000u) | fl;
    gstore<uint4>(e, hot);
    GF_WR(WR_HIT);
}

// ct_lookup4/6 (conntrack.h:310-437, dir = CT_INGRESS), resolve part: the home
// line of t (shared by the reverse-direction tuple t and the forward tuple tf
// under GF_HASH_CT) was loaded by the caller.  Reverse probe of t, then forward
// probe of tf, answered by one walk.  On return t holds the tuple the reference
// leaves in *tuple (tf unless the first probe hit), *tfl its flags, and pr the
// walk (its EMPTY slot is where ct_create inserts).
// DBG: *life receives the matched entry's lifetime as stored (DBG_CT_MATCH, conntrack.h:84)
template <int KSZ, int TW, int U, bool DBG = false>
__device__ __forceinline__ int ct_lookup(const gf_htab_desc &d, ProbeLine<KSZ, U, 4> &L, uint32_t *t, uint32_t nh,
                                         uint32_t &tfl, int action, bool syn, uint32_t len, uint32_t now, bool acct,
                                         CtState &st, ProbeRes &pr, uint32_t &ab, uint32_t *life = nullptr) {
    constexpr int AW = (TW - 2) / 2;                   // address words per side
    uint32_t tf[TW];
#pragma unroll
    for (int k = 0; k < AW; k++) { tf[k] = t[AW + k]; tf[AW + k] = t[k]; }
    tf[TW - 2] = (t[TW - 2] >> 16) | (t[TW - 2] << 16);
    tf[TW - 1] = nh | ((tfl ^ 1u) << 8);
    pr = probe2<KSZ, U, 4>(d, t, tf, L);
    ab += KSZ;
    uint4 hot = make_uint4(0, 0, 0, 0);
    if (pr.f >= 0) {
        constexpr int NW = Hdr<KSZ, 4>::NW;
        if (pr.u >= 0) {
#pragma unroll
            for (int u = 0; u < U; u++)
                if (u == pr.u) hot = make_uint4(L.hd[u].w[NW - 4], L.hd[u].w[NW - 3], L.hd[u].w[NW - 2], L.hd[u].w[NW - 1]);
        } else {
            hot = gload<uint4>(ht_val(d, (uint64_t)pr.f));
        }
    }
    if constexpr (DBG) *life = hot.x;
    if (pr.f >= 0 && !pr.is_b) {
        ct_hit(d, pr.f, hot, action, syn, len, now, acct, st, ab);
        return (tfl & 2u) ? CT_RELATED : CT_REPLY;
    }
    ab += KSZ;
#pragma unroll
    for (int k = 0; k < TW; k++) t[k] = tf[k];
    tfl ^= 1u;
    if (pr.f < 0) return CT_NEW;
    ct_hit(d, pr.f, hot, action, syn, len, now, acct, st, ab);
    return CT_ESTABLISHED;
}

// A slot in a log shared by many lanes: one atomic per wave (the active lanes'
// count), each lane its rank among them.
__device__ __forceinline__ uint32_t wave_reserve(uint32_t *ctr) {
    const uint64_t m = __ballot(1);
    const uint32_t lane = threadIdx.x & 63u, lead = (uint32_t)__ffsll((unsigned long long)m) - 1u;
    uint32_t base = 0;
    if (lane == lead) base = atomicAdd(ctr, (uint32_t)__popcll(m));
    base = __shfl(base, (int)lead);
    return base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
}
// One related-entry write into the run's set (RelSet).
__device__ __forceinline__ void rset_put(const RelSet &R, uint32_t w0, uint32_t w1, uint32_t side, uint32_t order) {
    const unsigned long long k = ((unsigned long long)w0 << 32) | w1;
    uint32_t p;
    const uint32_t want = order + 1u;
    uint32_t seen = 0;                                  // the key's word as last read (stale: lower)
    if (k == 0ull) {
        p = R.mask + 1u;
        if (atomicCAS(&R.slot[2ull * p], 0ull, 1ull) == 0ull) R.list[atomicAdd(R.list_n, 1u)] = p;
    } else {
        const uint32_t w[2] = {w0, w1};
        p = gf_hash_words(w, 2, 8) & R.mask;
        for (;;) {
            // plain read first (key and words together): within a run a key only goes
            // from 0 to its value and a word only up, so a stale read only makes the
            // CAS fail or costs the atomicMax it would have skipped
            const uint4 sl = *reinterpret_cast<const uint4 *>(R.slot + 2ull * p);
            unsigned long long cur = ((unsigned long long)sl.y << 32) | sl.x;
            if (cur == 0ull) {
                cur = atomicCAS(&R.slot[2ull * p], 0ull, k);
                if (cur == 0ull) { R.list[atomicAdd(R.list_n, 1u)] = p; break; }
            }
            if (cur == k) { seen = side ? sl.w : sl.z; break; }
            p = (p + 1u) & R.mask;
        }
    }
    if (seen < want) atomicMax(reinterpret_cast<uint32_t *>(R.slot + 2ull * p + 1u) + side, want);
}

// ct_create4/6 (conntrack.h:446-580) for ingress (ct_state->addr == 0).  The
// tuple goes to the EMPTY slot the lookup walk ended on (one CAS), the related
// entry to its cached slot when this lane wrote it before — or, with connection
// groups (rlog), to the log applied after the run.

template <int KSZ, int TW, int U>
__device__ __forceinline__ int ct_create(const gf_htab_desc &d, uint32_t *t, uint32_t rev_nat, uint32_t src_sec,
                                         uint32_t len, uint32_t now, bool strict, const ProbeRes &pr, int *added,
                                         RelCache<TW> &rc, uint32_t &ab, uint32_t *rlog = nullptr,
                                         uint32_t *rlog_n = nullptr, uint32_t order = 0, const RelSet *rs = nullptr) {
    constexpr int NHW = TW - 1;                         // word holding nexthdr | flags << 8
    ab += 2 * (KSZ + 48);                               // tuple + ICMP-related entry written
    uint32_t nh = t[NHW] & 0xffu, tfl = (t[NHW] >> 8) & 0xffu;
    uint32_t fl = (nh == 6) ? 0u : F_SEEN_NON_SYN;      // ct_update_timeout(syn = nexthdr == TCP)
    uint32_t life = now + ((fl & F_SEEN_NON_SYN) ? 43200u : 300u);
    // GF_VCODEC_CT: lifetime, flags|rev_nat, rx_packets/bytes lo, hi, tx, unused, src_sec_id
    uint32_t v[12] = {life, fl | (rev_nat << 16), 1u, len, 0u, 0u, 0u, 0u, 0u, 0u, 0u, src_sec};
    if (ht_upsert<KSZ, 12, GF_HASH_CT, U>(d, t, v, strict, added, true, pr.empty, pr.empty_word) < 0)
        return D_CT_CREATE_FAILED;
    uint32_t it[TW];
#pragma unroll
    for (int k = 0; k < TW; k++) it[k] = t[k];
    it[NHW - 1] = 0;                                    // sport = dport = 0
    it[NHW] = (KSZ == 40 ? 58u : 1u) | ((tfl | 2u) << 8);
    v[1] = (fl | F_SEEN_NON_SYN) | (rev_nat << 16);
    if constexpr (KSZ == 14) if (rlog) {                // connection groups: applied after the run, in order
        GF_WR(WR_RLOG);
        if (rs->slot) {
            rset_put(*rs, it[0], it[1], (it[NHW] >> 8) & 1u, order);
            return 0;
        }
        uint32_t *lg = rlog + (size_t)20 * wave_reserve(rlog_n);
        lg[0] = order;
#pragma unroll
        for (int k = 0; k < TW; k++) lg[1 + k] = it[k];
#pragma unroll
        for (int k = 0; k < 12; k++) lg[5 + k] = v[k];
        return 0;
    }
    bool same = rc.slot != ~0u;
#pragma unroll
    for (int k = 0; k < TW; k++) same &= ((k == TW - 1 ? rc.k[k] & 0x7fffu : rc.k[k]) == it[k]);
    if (same) {                                         // BPF_ANY over the entry this lane wrote
        if (d.vin == 16 && rc.sec == src_sec) {         // cold part (rx hi, tx, src_sec_id) unchanged
            if constexpr (TW == 4) {                    // (rev_nat is 0 on the ingress path)
                rc.k[3] = (rc.k[3] & 0x7fffu) | (((len << 1) | (nh == 6 ? 1u : 0u)) << 15);
            } else {
                store_words<4>(d.slots + (uint64_t)rc.slot * d.slot_size + d.voff, v);
                GF_WR(WR_REL_HOT);
            }
        } else {
            if constexpr (TW == 4) rc.k[3] &= 0x7fffu;  // superseded
            store_value<12>(d, (uint64_t)rc.slot, v);
            GF_WR(WR_REL_FULL);
        }
        rc.sec = src_sec;
        return 0;
    }
    if constexpr (TW == 4) rel_flush4(d, rc, now);      // the previous entry's pending write
    GF_WR(WR_REL_NEW);
    int64_t s = ht_upsert<KSZ, 12, GF_HASH_CT, U>(d, it, v, strict, added);
    if (s < 0) return D_CT_CREATE_FAILED;
#pragma unroll
    for (int k = 0; k < TW; k++) rc.k[k] = it[k];
    rc.slot = (uint64_t)s < 0xffffffffull ? (uint32_t)s : ~0u;
    rc.sec = src_sec;
    return 0;
}

// l4_proxy_lookup (ingress) + BPF_L4_MAP semantics, bpf/lib/l4.h:151-217, common.h:105-127
__device__ __forceinline__ int l4_proxy_lookup(const gf_lxc_dev *c, uint32_t nh, uint32_t dport) {
    if (nh != 6 && nh != 17) return 0;
    uint32_t n = gload<uint32_t>(&c->n_l4);
    if (!n) return 0;
    for (uint32_t k = 0; k < n; k++) {
        gf_l4_allow_dev a = gload<gf_l4_allow_dev>(&c->l4[k]);
        if (a.port && a.port == dport) {
            if (a.nexthdr && a.nexthdr == nh) return a.proxy;   // first match decides
        }
    }
    return 0;
}

// policy_entry packets/bytes counters (policy.h:67-68,79-80,91-92).  The
// reference adds them per packet; nothing reads them inside a batch (the host
// sees them after classify returns), so a lane sums the increments of its
// consecutive packets that hit the same entry in registers and applies them
// with one pair of atomics when the entry changes and at the end — the same
// totals with a fraction of the memory-side atomics.
// policy_entry packets += pk, bytes += by at c (two u64 atomics; agent-scope atomics
// go to the memory side, ~17 G/s on MI355X).  wave (IngCtx::pol_wave): the active
// lanes that add to the same entry as the first active lane sum their counts in
// registers first and that lane adds once; the other lanes add their own.  It pays
// on the egress deliveries' pass, whose lanes take neighbouring packets of few
// endpoints (deliveries' k_ing_groups 0.662 -> 0.625 ms), and costs the ingress
// configurations, whose lanes rarely share an entry (config 2 2.535 -> 2.565 ms,
// config 4 1.902 -> 1.957: profiles/r5q_*.json).  Counter sums commute: the final
// values are the reference's.
__device__ __forceinline__ void pol_count_add(uint8_t *c, uint32_t pk, uint32_t by, bool wave) {
  if (wave) {
    const uint64_t act = __ballot(1);
    const uint32_t lane = threadIdx.x & 63u, lead = (uint32_t)__ffsll((unsigned long long)act) - 1u;
    const uint64_t lc = (uint64_t)(uintptr_t)c;
    const uint32_t clo = (uint32_t)__shfl((int)(uint32_t)lc, (int)lead);
    const uint32_t chi = (uint32_t)__shfl((int)(uint32_t)(lc >> 32), (int)lead);
    const bool same = (uint32_t)lc == clo && (uint32_t)(lc >> 32) == chi;
    const uint64_t m = __ballot(same) & act;
    if (same) {                                         // (only the lanes of m run this: sources active)
        unsigned long long sp = 0, sb = 0;
        for (uint64_t mm = m; mm; mm &= mm - 1ull) {
            const int l = __ffsll((unsigned long long)mm) - 1;
            sp += (uint32_t)__shfl((int)pk, l);
            sb += (uint32_t)__shfl((int)by, l);
        }
        if (lane == lead) { gadd64(c, sp); gadd64(c + 8, sb); }
        return;
    }
  }
    gadd64(c, (unsigned long long)pk);
    gadd64(c + 8, (unsigned long long)by);
}
struct PolAcc {
    uint32_t f[2];                           // policy slots of the open sums
    uint16_t sl[2];                          // their program slot + 1 (0: sum not open)
    uint32_t pk[2], by[2];                   // flushed before a 32-bit sum could wrap
    __device__ __forceinline__ void init() {
        for (int j = 0; j < 2; j++) { f[j] = 0; sl[j] = 0; pk[j] = 0; by[j] = 0; }
    }
    __device__ __forceinline__ void flush_one(const IngCtx &X, int j) {
        if (sl[j]) {
            uint8_t *side = gload<uint8_t *>(&X.cfgs[sl[j] - 1].policy.vals);
            uint8_t *c = side + (uint64_t)f[j] * GF_POL_SIDE;
            pol_count_add(c, pk[j], by[j], X.pol_wave != 0);
            GF_WR(WR_POLCNT); GF_WR(WR_POLCNT);
        }
        sl[j] = 0; pk[j] = 0; by[j] = 0;
    }
    __device__ __forceinline__ void flush(const IngCtx &X) { flush_one(X, 0); flush_one(X, 1); }
    __device__ __forceinline__ void add(const IngCtx &X, uint32_t s, uint32_t slot, uint32_t len, uint32_t &next) {
        int j = (sl[0] == s && f[0] == slot) ? 0 : ((sl[1] == s && f[1] == slot) ? 1 : -1);
        if (j < 0) { j = (int)(next & 1u); next ^= 1u; flush_one(X, j); sl[j] = (uint16_t)s; f[j] = slot; }
        else if (by[j] + len < by[j] || pk[j] == 0xffffffffu) { flush_one(X, j); sl[j] = (uint16_t)s; f[j] = slot; }
        pk[j] += 1u; by[j] += len;
    }
};

// policy_entry packets/bytes of slot f of the program's policy map (policy maps
// hold < 2^32 slots: max_entries is u32 and the load is <= 1/2)
__device__ __forceinline__ void policy_count(const IngCtx &X, Ep &ep, int64_t f, uint32_t len, PolAcc &acc) {
    acc.add(X, ep.sl, (uint32_t)f, len, ep.next);
}

// A policy slot is 16 B with proxy_port inside, so an L4 hit needs no second load.
typedef ProbeLine<8, GF_POL_U, 0> PolLine;

__device__ __forceinline__ uint32_t pol_home(uint32_t identity, uint32_t dport, uint32_t proto) {
    uint32_t kw[2] = {identity, dport | (proto << 16)};
    return key_hash<8, GF_HASH_POLICY>(kw);
}

// The lane's last policy decision.  __policy_can_access + the reserved-identity
// CIDR check are a pure function of (program, identity, dport, proto, source
// address for reserved identities) while a batch runs: the device never changes
// policy keys, proxy ports, CIDR tries or L4 lists, only the entry counters —
// which stay per packet.  Consecutive packets of a lane's flow group mostly ask
// the same question, so the answer (and the entry to count) is kept.
struct PolDecision {          // 24 B (kept in LDS with the rest of the lane state)
    uint32_t id, sip, pk;
    uint32_t slab;           // program slot + 1 | algorithmic bytes of the decision << 16 (0: empty)
    uint32_t f;              // policy slot counted by the decision, ~0u: none
    int verdict;
};
template <int N>
struct PolMemo {             // N decisions (a group's flows use a couple of ports)
    PolDecision d[N];
    __device__ __forceinline__ void init() {
#pragma unroll
        for (int j = 0; j < N; j++) d[j].slab = 0;
    }
    __device__ __forceinline__ int find(uint32_t s, uint32_t identity, uint32_t k, uint32_t a) const {
#pragma unroll
        for (int j = 0; j < N; j++)
            if ((d[j].slab & 0xffffu) == s && d[j].id == identity && d[j].pk == k && (identity >= 256 || d[j].sip == a))
                return j;
        return -1;
    }
    __device__ __forceinline__ bool hit(uint32_t s, uint32_t identity, uint32_t k, uint32_t a) const {
        return find(s, identity, k, a) >= 0;
    }
    // the slot a new decision replaces: round-robin on bit 1 of the endpoint's bits
    __device__ __forceinline__ PolDecision &victim(uint32_t &next) {
        if constexpr (N == 1) return d[0];
        PolDecision &v = d[(next >> 1) & 1u];
        next ^= 2u;
        return v;
    }
};

// __policy_can_access (policy.h:42-113) + policy_can_access_ingress (:133-168),
// without the counter update: *fc = the entry the reference counts (or -1).
// pl: the home line of (identity, *) if pl_loaded (identity != 0 hashes by
// identity only, so the L4 and the L3 key of the identity share it).
__device__ int policy_lookup(const IngCtx &X, const Ep &ep, PolLine &pl, bool pl_loaded, uint32_t identity, uint32_t dport,
                             uint32_t proto, bool v6, const uint32_t *cidr_addr, uint32_t &ab, int64_t &fc) {
    const uint32_t flags = ep.flags;
    fc = -1;
    if (flags & GF_LXC_F_DROP_ALL) return D_POLICY;
    if (!(flags & GF_LXC_F_POLICY_INGRESS)) return TC_OK;
    const gf_htab_desc pd = ep.pdesc();
    int64_t f;
    uint32_t pp = 0;
    {
        uint32_t k4[2] = {identity, dport | (proto << 16)}, k3[2] = {identity, 0u};
        if (!pl_loaded) pl.load(pd, identity ? pol_home(identity, 0u, 0u) : pol_home(0u, dport, proto));
        if (flags & GF_LXC_F_HAVE_L4_POLICY) {
            ProbeRes r = probe2<8, GF_POL_U, 0>(pd, k4, k3, pl, identity != 0);
            ab += 8;
            if (r.f >= 0 && !r.is_b) {
                pp = 0xffffffffu;
#pragma unroll
                for (int u = 0; u < GF_POL_U; u++)
                    if (u == r.u) pp = pl.hd[u].w[2] >> 16;          // proxy_port at slot byte 10
                f = r.f;
                goto proxy;
            }
            ab += 8;
            if (!identity) {                                // L3 key {0,0,0}: its own home line
                f = ht_find<8, GF_POL_U>(pd, k3, key_hash<8, GF_HASH_POLICY>(k3));
            } else f = r.f;
            if (f >= 0) { ab += 40; fc = f; return TC_OK; }
        } else {
            if (identity) { ProbeRes r = probe2<8, GF_POL_U, 0>(pd, k3, k3, pl, false); f = r.f; }
            else f = ht_find<8, GF_POL_U>(pd, k3, key_hash<8, GF_HASH_POLICY>(k3));
            ab += 8;
            if (f >= 0) { ab += 40; fc = f; return TC_OK; }
        }
    }
    if (flags & GF_LXC_F_HAVE_L4_POLICY) {
        uint32_t kw[2] = {0u, dport | (proto << 16)};
        f = ht_find<8, GF_POL_U>(pd, kw, key_hash<8, GF_HASH_POLICY>(kw));
        ab += 8;
        if (f >= 0) { pp = 0xffffffffu; goto proxy; }
    }
    goto deny;
proxy: {
        ab += 40;                                       // entry read + counters written
        fc = f;
        if (pp == 0xffffffffu) pp = gload<uint16_t>(ht_val(pd, (uint64_t)f));
        if (pp) return (int)pp;
        return l4_proxy_lookup(ep.cfg(X), proto, dport);
    }
deny:
    if (identity < 256) {                               // identity_is_reserved
        const gf_lxc_dev *c = ep.cfg(X);
        if (v6) { const gf_trie_desc tr = gload<gf_trie_desc>(&c->cidr6); if (tr.root_bits) ab += 21; if (trie_lookup<4>(tr, cidr_addr)) return TC_OK; }
        else { const gf_trie_desc tr = gload<gf_trie_desc>(&c->cidr4); if (tr.root_bits) ab += 9; if (trie_lookup<1>(tr, cidr_addr)) return TC_OK; }
    }
    return D_POLICY;
}

// Debug notifications (bpf/lib/dbg.h, DEBUG; GF_LXC_F_DEBUG).  Like the traces,
// the records are written by the event pass; the debug instantiation of
// k_ing_groups leaves, per packet of a program with the flag, what neither the
// verdict record nor gf_rec nor the program can tell: one 32-B entry.
//   w0  GF_DBG_* bits: the messages handle_policy sent | l4_proxy_lookup's result << 16
//   w1  DBG_CT_MATCH: entry->lifetime as stored when the lookup found it
//   w2  the matched entry's rev_nat_index (== ct_state.rev_nat_index at DBG_CT_VERDICT)
//   w3  ct_lookup's return value
//   w4  the dport the policy was asked with (tuple.dport after the lookup, raw be16)
//   w5  the redirect's new_port (raw be16; the record loses it on DROP_PROXYMAP_CREATE_FAILED)
//   w6, w7  IPv6: tuple.saddr.p4, tuple.daddr.p4 (DBG_CT_LOOKUP6_1; daddr.p4 & 0xffff is
//       DBG_CT_CREATED6's rev_nat_index)
// An entry of all zeros expands to nothing (the column is cleared before the launch).
#define GF_DBG_LOOKUP   (1u << 0)   // ct_lookup reached its first message: LOOKUP*_1, LOOKUP*_2, CT_VERDICT
#define GF_DBG_SKIP     (1u << 1)   // DBG_SKIP_PROXY
#define GF_DBG_MATCH    (1u << 2)   // DBG_CT_MATCH
#define GF_DBG_L4_KEY   (1u << 3)   // DBG_L4_CREATE: the {identity, dport, proto} key hit
#define GF_DBG_L4_PROXY (1u << 4)   // l4_proxy_lookup ran: DBG_GENERIC, DBG_L4_POLICY
#define GF_DBG_DENIED   (1u << 5)   // DBG_POLICY_DENIED
#define GF_DBG_CREATED  (1u << 6)   // DBG_CT_CREATED4/6 (sent before the map update)
#define GF_DBG_CAPTURE  (1u << 7)   // the redirect got to DBG_CAPTURE_PROXY_POST (IPv4: + DBG_REV_PROXY_UPDATE)
// LB_DEBUG (GF_LXC_F_LB_DEBUG; cilium_dbg_lb, lb.h:85-89).  The index looked up is w2; nat->address /
// nat->port are not logged: the event pass finds them again from w2 (the reverse-NAT maps are
// host-managed and cannot change inside a call), so the log stays 32 B.
#define GF_DBG_REVNAT     (1u << 8)   // lb{4,6}_rev_nat was entered: DBG_LB{4,6}_REVERSE_NAT_LOOKUP (lb.h:310, 531)
#define GF_DBG_REVNAT_HIT (1u << 9)   // the lookup hit, __lb{4,6}_rev_nat ran: DBG_LB{4,6}_REVERSE_NAT (lb.h:264, 456)
struct DbgLog {
    uint32_t w[8];
    __device__ __forceinline__ void init() {
#pragma unroll
        for (int k = 0; k < 8; k++) w[k] = 0;
    }
};
// The memo keeps which key answered in two spare bits of PolDecision::slab (the
// algorithmic bytes of a decision stay far below 2^14): debug instantiation only.
#define GF_MEMO_DBG_L4_KEY   (1u << 30)
#define GF_MEMO_DBG_L4_PROXY (1u << 31)
// Which key of __policy_can_access answered (policy.h:60-108), from the entry it
// counted: slot fc of the program's policy map (key words 0-1, proxy_port at byte 10).
__device__ __attribute__((noinline)) uint32_t pol_dbg_key_ol(const uint8_t *slot, uint32_t identity, uint32_t pk,
                                                             uint32_t proto) {
    const uint4 e = gload<uint4>(slot);
    if (e.y == 0u) return 0u;                           // the L3 key {identity, 0, 0}: no message
    uint32_t b = 0;
    if (e.x == identity && e.y == pk) b |= GF_MEMO_DBG_L4_KEY;     // the first lookup (also when identity is 0)
    if (!(e.z >> 16) && (proto == 6 || proto == 17)) b |= GF_MEMO_DBG_L4_PROXY;   // proxy_port 0: l4_proxy_lookup
    return b;
}

// policy_can_access_ingress with the counter update (policy.h:67-92), through the
// lane's decision memo (IPv4, or any non-reserved identity).
// DBG: *dk receives the GF_DBG_L4_KEY / L4_PROXY / DENIED bits of the decision.
template <int N, bool DBG = false>
__device__ __forceinline__ int policy_ingress(const IngCtx &X, Ep &ep, PolLine &pl, bool pl_loaded, uint32_t identity,
                                              uint32_t dport, uint32_t proto, uint32_t len, bool v6,
                                              const uint32_t *cidr_addr, uint32_t &ab, PolAcc &acc, PolMemo<N> &m,
                                              uint32_t *dk = nullptr) {
    const uint32_t pk = dport | (proto << 16), sip = v6 ? 0u : cidr_addr[0];
    const bool memo_ok = !v6 || identity >= 256;
    const int j = memo_ok ? m.find(ep.sl, identity, pk, sip) : -1;
    if (j >= 0) {
        const PolDecision &d = m.d[j];
        if constexpr (DBG) {
            ab += (d.slab >> 16) & 0x3fffu;
            *dk = ((d.slab & GF_MEMO_DBG_L4_KEY) ? GF_DBG_L4_KEY : 0u) | ((d.slab & GF_MEMO_DBG_L4_PROXY) ? GF_DBG_L4_PROXY : 0u) |
                  (d.verdict < 0 ? GF_DBG_DENIED : 0u);
        } else {
            ab += d.slab >> 16;
        }
        if (d.f != ~0u) policy_count(X, ep, (int64_t)d.f, len, acc);
        return d.verdict;
    }
    uint32_t ab0 = ab;
    int64_t fc;
    int v = policy_lookup(X, ep, pl, pl_loaded, identity, dport, proto, v6, cidr_addr, ab, fc);
    if (fc >= 0) policy_count(X, ep, fc, len, acc);
    uint32_t mk = 0;
    if constexpr (DBG) {
        // (no message without POLICY_INGRESS: policy_can_access_ingress is the stub, policy.h:170-178)
        if (fc >= 0 && (ep.flags & GF_LXC_F_HAVE_L4_POLICY))
            mk = pol_dbg_key_ol(ep.pol + (uint64_t)fc * GF_POL_SLOT, identity, pk, proto);
        *dk = ((mk & GF_MEMO_DBG_L4_KEY) ? GF_DBG_L4_KEY : 0u) | ((mk & GF_MEMO_DBG_L4_PROXY) ? GF_DBG_L4_PROXY : 0u) |
              (v < 0 ? GF_DBG_DENIED : 0u);
    }
    if (memo_ok) {
        PolDecision &d = m.victim(ep.next);
        d.id = identity; d.pk = pk; d.sip = sip; d.verdict = v;
        d.f = fc >= 0 ? (uint32_t)fc : ~0u;    // policy maps hold < 2^32 slots (max_entries is u32)
        d.slab = ep.sl | ((ab - ab0) << 16) | mk;
    }
    return v;
}

// __lb{4,6}_rev_nat verdict-affecting checks (lb.h:217-293, 447-512)
__device__ __forceinline__ int rev_nat_checks(uint32_t len, int l4_off, uint32_t nh, uint32_t nat_port,
                                              uint32_t l4w0, bool v6) {
    uint32_t co = csum_l4_offset(nh);
    if (nat_port) {
        if (nh == 6 || nh == 17) {
            if (!skb_ok(l4_off, 2, len)) return -GF_EFAULT;
            if (nat_port != (l4w0 & 0xffffu)) {
                if (!l4csum_ok(l4_off + (int)co, len)) return D_CSUM_L4;
                if (!skb_ok(l4_off, 2, len)) return D_WRITE_ERROR;
            }
        } else if (nh != 1 && nh != 58) return D_UNKNOWN_L4;
    }
    if (v6) { if (!l4csum_ok(l4_off + (int)co, len)) return D_CSUM_L4; }
    else if (co && !l4csum_ok(l4_off + (int)co, len)) return D_CSUM_L4;
    return 0;
}

// ipv{4,6}_redirect_to_host_port verdict-affecting checks (lib/lxc.h:96-205)
__device__ __forceinline__ int redirect_checks(uint32_t len, int l4_off, uint32_t nh) {
    uint32_t co = csum_l4_offset(nh);
    if (!l4csum_ok(l4_off + (int)co, len)) return D_WRITE_ERROR;
    if (!skb_ok(l4_off + 2, 2, len)) return D_WRITE_ERROR;
    return 0;
}

// ct_lookup4/6 header part: fills tuple port/flag words, returns action or error
__device__ __forceinline__ int ct_l4(uint32_t nh, bool v6, const gf_rec &r, uint32_t &pw, uint32_t &tfl,
                                     int &action, bool &syn) {
    uint32_t len = r.len;
    int off = r.l4_off;
    action = ACT_UNSPEC; syn = false;
    if ((!v6 && nh == 1) || (v6 && nh == 58)) {
        if (!skb_ok(off, 1, len)) return D_CT_INVALID_HDR;
        uint32_t type = r.l4w0 & 0xffu;
        pw = 0;
        if (!v6) {
            if (type == 3 || type == 11 || type == 12) tfl |= 2u;
            else if (type == 0) pw = 8u;                         // dport = ICMP_ECHO
            else { if (type == 8) pw = 8u << 16; action = ACT_CREATE; }
        } else {
            if (type >= 1 && type <= 4) tfl |= 2u;
            else if (type == 129) pw = 128u;
            else { if (type == 128) pw = 128u << 16; action = ACT_CREATE; }
        }
        return 0;
    }
    if (nh == 6) {
        if (!skb_ok(off + 12, 2, len)) return D_CT_INVALID_HDR;
        uint32_t w = r.l4w3;
        bool fin = (w >> 8) & 1, sy = (w >> 9) & 1, rst = (w >> 10) & 1;
        action = (rst || fin) ? ACT_CLOSE : ACT_CREATE;
        syn = sy;
        if (!skb_ok(off, 4, len)) return D_CT_INVALID_HDR;
        pw = r.l4w0;
        return 0;
    }
    if (nh == 17) {
        if (!skb_ok(off, 4, len)) return D_CT_INVALID_HDR;
        pw = r.l4w0;
        action = ACT_CREATE;
        return 0;
    }
    return D_CT_UNKNOWN_PROTO;
}

// Out-of-line copies for the IPv6 kernel, whose register budget the inlined
// cold paths would cut to 2 waves/SIMD (the IPv4 kernel keeps them inline).
__device__ __attribute__((noinline)) void pol_rev_nat_write_ol(PolCtx X, uint32_t i, uint32_t len, int l4_off,
                                                               uint32_t nh, const uint8_t *nat) {
    pol_rev_nat_write(X, i, len, l4_off, nh, nat, true, 0u);
}
__device__ __attribute__((noinline)) void pol_v6_zero_rn_ol(PolCtx X, uint32_t i, uint32_t len, int l4_off,
                                                            uint32_t nh, uint32_t rn) {
    pol_v6_zero_rn(X, i, len, l4_off, nh, rn);
}
struct V6Tuple { uint32_t w[10]; };
__device__ __attribute__((noinline)) void pol_redirect_ol(PolCtx X, uint32_t i, uint32_t len, int l4_off,
                                                          uint32_t nh, V6Tuple t, uint32_t new_port,
                                                          uint4 od, uint32_t identity) {
    const uint32_t odw[4] = {od.x, od.y, od.z, od.w};
    pol_redirect(X, i, len, l4_off, nh, t.w, true, new_port, odw, identity);
}

// ipv4_policy, bpf/bpf_lxc.c:865-970
// rlog: X.rlog unless the run fell back to pair groups (read once per kernel, k_ing_groups);
// RL: the instance has the egress connection groups' related-entry path at all (the
// egress deliveries' pass), kept out of the others' registers
// DBG: the debug instantiation fills *dl (DbgLog) as the messages are sent
template <bool PCT, bool RL = false, bool DBG = false>
__device__ int ipv4_policy(const IngCtx &X, Ep &ep, const gf_rec &r, uint32_t i, int &fwd, uint8_t &ofl, uint16_t &proxy,
                           uint32_t &ifindex, int *added, uint32_t &ab, PolAcc &acc, RelCache<4> &rc, PolMemo<GF_MEMO4> &pm,
                           uint32_t *rlog, DbgLog *dl = nullptr) {
    uint32_t len = r.len;
    if (len < 34) return D_INVALID;
    const uint32_t flags = ep.flags;
    if constexpr (DBG) if (r.cls & 4) dl->w[0] |= GF_DBG_SKIP;   // tc_index_skip_proxy (lxc.h:196-205)
    uint32_t nh = r.proto;
    uint32_t t[4] = {r.daddr, r.saddr, 0u, nh};
    uint32_t tfl = 0;                                   // TUPLE_F_OUT (ingress)
    if (nh == 1) {                                      // its related probe may read the pending entry
        if constexpr (PCT) rel_flush4(ing_ct<4, true>(X, ep), rc, X.now);   // (the lane's cache is this map's)
        else rel_flush4(X.ct4, rc, X.now);
    }
    int action; bool syn;
    int e = ct_l4(nh, false, r, t[2], tfl, action, syn);
    if (e < 0) return e;
    t[3] = nh | (tfl << 8);
    const gf_htab_desc ct = ing_ct<4, PCT>(X, ep);
    // the CT home line and the policy home line of the source identity go out together
    ProbeLine<14, GF_CT4_U, 4> cl;
#if GF_CT_COOP
    cl.load_quad(ct, key_hash<14, GF_HASH_CT>(t));
#else
    cl.load(ct, key_hash<14, GF_HASH_CT>(t));
#endif
    // (unless the lane's policy memo already answers the NEW/ESTABLISHED question)
    PolLine pl;
    const bool pre = r.src_identity &&
                     (flags & (GF_LXC_F_POLICY_INGRESS | GF_LXC_F_DROP_ALL)) == GF_LXC_F_POLICY_INGRESS &&
                     !pm.hit(ep.sl, r.src_identity, (t[2] >> 16) | (nh << 16), r.saddr);
    if (pre) pl.load(ep.pdesc(), pol_home(r.src_identity, 0u, 0u));
    bool acct = (flags & GF_LXC_F_CT_ACCOUNTING) != 0;
    CtState st{0, 0, 0};
    ProbeRes pr;
    int ret;
    if constexpr (DBG) {
        ret = ct_lookup<14, 4, GF_CT4_U, true>(ct, cl, t, nh, tfl, action, syn, len, X.now, acct, st, pr, ab, &dl->w[1]);
        dl->w[0] |= GF_DBG_LOOKUP | (ret != CT_NEW ? GF_DBG_MATCH : 0u);
        dl->w[2] = st.rev_nat; dl->w[3] = (uint32_t)ret;
    } else {
        ret = ct_lookup<14, 4, GF_CT4_U>(ct, cl, t, nh, tfl, action, syn, len, X.now, acct, st, pr, ab);
    }
    fwd = ret;
    if (st.carry) rel_drop(PCT ? ct : X.ct4, rc, X.now);   // a counter carry touched a cold value part
    if (ret == CT_REPLY && st.rev_nat && !st.loopback) {
        const gf_htab_desc rn = gload<gf_htab_desc>(&ep.cfg(X)->revnat4);
        uint32_t kw[1] = {st.rev_nat};
        int64_t f = ht_find<2>(rn, kw, key_hash<2>(kw));
        ab += 8;
        if constexpr (DBG) dl->w[0] |= GF_DBG_REVNAT | (f >= 0 ? GF_DBG_REVNAT_HIT : 0u);   // (sent before any check fails)
        if (f >= 0) {
            const uint8_t *nat = ht_val(rn, f);
            int r2 = rev_nat_checks(len, r.l4_off, nh, gload<uint16_t>(nat + 4), r.l4w0, false);
            if (r2 < 0) return r2;
            if (X.snap) pol_rev_nat_write(X, i, len, r.l4_off, nh, nat, false, t[1]);
            t[1] = gload<uint32_t>(nat);                       // tuple->saddr = nat->address
        }
    }
    uint32_t orig_sip = r.saddr;
    int verdict;
    if constexpr (DBG) {
        uint32_t dk = 0;
        verdict = policy_ingress<GF_MEMO4, true>(X, ep, pl, pre, r.src_identity, t[2] & 0xffffu, nh, len, false, &orig_sip, ab,
                                                 acc, pm, &dk);
        dl->w[0] |= dk | ((dk & GF_DBG_L4_PROXY) ? (uint32_t)verdict << 16 : 0u);
        dl->w[4] = t[2] & 0xffffu;
    } else {
        verdict = policy_ingress(X, ep, pl, pre, r.src_identity, t[2] & 0xffffu, nh, len, false, &orig_sip, ab, acc, pm);
    }
    if (ret != CT_REPLY && ret != CT_RELATED && verdict < 0) {
        if (ret == CT_ESTABLISHED) {
            ab += 14;
            ht_delete<14, GF_HASH_CT, GF_CT4_U>(ct, t, X.strict & 1, added);
            rel_drop(PCT ? ct : X.ct4, rc, X.now);
        }
        return D_POLICY;
    }
    if (r.cls & 4) verdict = 0;                         // skip_proxy
    if (ret == CT_NEW) {
        if constexpr (DBG) dl->w[0] |= GF_DBG_CREATED;
        ret = ct_create<14, 4, GF_CT4_U>(ct, t, 0u, r.src_identity, len, X.now, X.strict & 1, pr, added, rc, ab,
                                         RL ? rlog : nullptr, X.rlog_n, 2u * i + 1u, &X.rs);
        if (ret < 0) return ret;
        ofl |= GF_INGRESS_F_CREATED;
    }
    if (verdict > 0 && (ret == CT_NEW || ret == CT_ESTABLISHED)) {
        if (X.tmark)
            trace_proxy(X.tmark, X.tcap, X.snap ? X.snap + (size_t)i * X.snap_stride : nullptr, nullptr, 0,
                        trace_cap_len(len, X.snap_stride), i, GF_TR_PX_POLICY);
        int r3 = redirect_checks(len, r.l4_off, nh);
        if (r3 < 0) return r3;
        if constexpr (DBG) { dl->w[0] |= GF_DBG_CAPTURE; dl->w[5] = (uint32_t)verdict & 0xffffu; }
        if (X.snap || X.plog) { const uint32_t od[1] = {r.daddr}; pol_redirect(X, i, len, r.l4_off, nh, t, false, (uint32_t)verdict & 0xffffu, od, r.src_identity); }
        ifindex = X.host_ifindex;
        ofl |= GF_INGRESS_F_PROXY;
        proxy = (uint16_t)verdict;
    }
    return 0;
}

// ipv6_policy, bpf/bpf_lxc.c:745-862
template <bool PCT, bool DBG = false>
__device__ int ipv6_policy(const IngCtx &X, Ep &ep, const gf_rec &r, uint32_t i, int &fwd, uint8_t &ofl,
                           uint16_t &proxy, uint32_t &ifindex, int *added, uint32_t &ab, PolAcc &acc,
                           RelCache<10> &rc, PolMemo<GF_MEMO6> &pm, DbgLog *dl = nullptr) {
    uint32_t len = r.len;
    if (len < 54) return D_INVALID;
    if (!X.daddr6 || !X.saddr6) return D_INVALID;      // batch built without IPv6 columns
    const uint32_t flags = ep.flags;
    if constexpr (DBG) if (r.cls & 4) dl->w[0] |= GF_DBG_SKIP;   // tc_index_skip_proxy (lxc.h:196-205)
    uint32_t nh = r.proto;
    uint4 d = gload<uint4>(X.daddr6 + (size_t)X.a6_stride * i);
    uint4 s = gload<uint4>(X.saddr6 + (size_t)X.a6_stride * i);
    uint32_t t[10] = {d.x, d.y, d.z, d.w, s.x, s.y, s.z, s.w, 0u, nh};
    uint32_t co = csum_l4_offset(nh);
    uint32_t rn_new = d.w & 0xffffu;                    // ip6->daddr.s6_addr32[3] & 0xFFFF
    if (rn_new) {
        if (X.snap) pol_v6_zero_rn_ol(pol_ctx(X), i, len, r.l4_off, nh, rn_new);
        if (co && !l4csum_ok(r.l4_off + (int)co, len)) return D_CSUM_L4;
    }
    uint32_t tfl = 0;
    int action; bool syn;
    int e = ct_l4(nh, true, r, t[8], tfl, action, syn);
    if (e < 0) return e;
    t[9] = nh | (tfl << 8);
    const gf_htab_desc ct = ing_ct<6, PCT>(X, ep);
    ProbeLine<40, GF_CT6_U, 4> cl;
#if GF_CT_COOP6
    cl.load_quad(ct, key_hash<40, GF_HASH_CT>(t));
#else
    cl.load(ct, key_hash<40, GF_HASH_CT>(t));
#endif
    PolLine pl;
    const bool pre = r.src_identity &&
                     (flags & (GF_LXC_F_POLICY_INGRESS | GF_LXC_F_DROP_ALL)) == GF_LXC_F_POLICY_INGRESS &&
                     !(r.src_identity >= 256 && pm.hit(ep.sl, r.src_identity, (t[8] >> 16) | (nh << 16), 0u));
    if (pre) pl.load(ep.pdesc(), pol_home(r.src_identity, 0u, 0u));
    bool acct = (flags & GF_LXC_F_CT_ACCOUNTING) != 0;
    CtState st{0, 0, 0};
    ProbeRes pr;
    int ret;
    if constexpr (DBG) {
        dl->w[6] = s.w; dl->w[7] = d.w;
        ret = ct_lookup<40, 10, GF_CT6_U, true>(ct, cl, t, nh, tfl, action, syn, len, X.now, acct, st, pr, ab, &dl->w[1]);
        dl->w[0] |= GF_DBG_LOOKUP | (ret != CT_NEW ? GF_DBG_MATCH : 0u);
        dl->w[2] = st.rev_nat; dl->w[3] = (uint32_t)ret;
    } else {
        ret = ct_lookup<40, 10, GF_CT6_U>(ct, cl, t, nh, tfl, action, syn, len, X.now, acct, st, pr, ab);
    }
    fwd = ret;
    if (st.carry) rc.slot = ~0u;
    if (st.rev_nat) {
        const gf_htab_desc rn = gload<gf_htab_desc>(&ep.cfg(X)->revnat6);
        uint32_t kw[1] = {st.rev_nat};
        int64_t f = ht_find<2>(rn, kw, key_hash<2>(kw));
        ab += 20;
        if constexpr (DBG) dl->w[0] |= GF_DBG_REVNAT | (f >= 0 ? GF_DBG_REVNAT_HIT : 0u);   // (sent before any check fails)
        if (f >= 0) {
            const uint8_t *nat = ht_val(rn, f);
            int r2 = rev_nat_checks(len, r.l4_off, nh, gload<uint16_t>(nat + 16), r.l4w0, true);
            if (r2 < 0) return r2;
            if (X.snap) pol_rev_nat_write_ol(pol_ctx(X), i, len, r.l4_off, nh, nat);
        }
    }
    int verdict;
    if constexpr (DBG) {
        uint32_t dk = 0;
        verdict = policy_ingress<GF_MEMO6, true>(X, ep, pl, pre, r.src_identity, t[8] & 0xffffu, nh, len, true, t + 4, ab, acc,
                                                 pm, &dk);
        dl->w[0] |= dk | ((dk & GF_DBG_L4_PROXY) ? (uint32_t)verdict << 16 : 0u);
        dl->w[4] = t[8] & 0xffffu;
    } else {
        verdict = policy_ingress(X, ep, pl, pre, r.src_identity, t[8] & 0xffffu, nh, len, true, t + 4, ab, acc, pm);
    }
    if (ret != CT_REPLY && ret != CT_RELATED && verdict < 0) {
        if (ret == CT_ESTABLISHED) {
            ab += 40;
            ht_delete<40, GF_HASH_CT, GF_CT6_U>(ct, t, (X.strict & 2) != 0, added);
            rc.slot = ~0u;
        }
        return D_POLICY;
    }
    if (r.cls & 4) verdict = 0;
    if (ret == CT_NEW) {
        if constexpr (DBG) dl->w[0] |= GF_DBG_CREATED;
        ret = ct_create<40, 10, GF_CT6_U>(ct, t, rn_new, r.src_identity, len, X.now, (X.strict & 2) != 0, pr, added, rc, ab);
        if (ret < 0) return ret;
        ofl |= GF_INGRESS_F_CREATED;
    }
    if (verdict > 0 && (ret == CT_NEW || ret == CT_ESTABLISHED)) {
        if (X.tmark)
            trace_proxy(X.tmark, X.tcap, X.snap ? X.snap + (size_t)i * X.snap_stride : nullptr, nullptr, 0,
                        trace_cap_len(len, X.snap_stride), i, GF_TR_PX_POLICY);
        int r3 = redirect_checks(len, r.l4_off, nh);
        if (r3 < 0) return r3;
        if constexpr (DBG) { dl->w[0] |= GF_DBG_CAPTURE; dl->w[5] = (uint32_t)verdict & 0xffffu; }
        if (X.snap || X.plog) {
            V6Tuple tv;
#pragma unroll
            for (int k = 0; k < 10; k++) tv.w[k] = t[k];
            pol_redirect_ol(pol_ctx(X), i, len, r.l4_off, nh, tv, (uint32_t)verdict & 0xffffu, d, r.src_identity);
        }
        ifindex = X.host_ifindex;
        ofl |= GF_INGRESS_F_PROXY;
        proxy = (uint16_t)verdict;
    }
    return 0;
}

// Per-lane state carried across the packets of the lane's buckets.  It lives in
// LDS (one record per thread, k_ing_groups) so that registers hold only the
// state of the packet in flight: the register budget is what bounds waves per
// SIMD, and waves in flight are what hide the probes' memory latency.
// The lane's share of the counter block: wire / algorithmic byte sums and the
// four CT-result counts (16 bits each; the packet count is their sum), kept per
// lane so the common bins take no same-address LDS atomics; folded into the
// block's bins before a field could wrap and at the end of the launch.
struct LaneCnt {
    uint32_t len, ab, c01, c23;
    __device__ __forceinline__ void init() { len = ab = c01 = c23 = 0; }
    __device__ __forceinline__ void fold(Stats &st) {
        const uint32_t a = c01 & 0xffffu, b = c01 >> 16, c = c23 & 0xffffu, d = c23 >> 16;
        st.add_n(264, a); st.add_n(265, b); st.add_n(266, c); st.add_n(267, d);
        st.add_n(268, a + b + c + d); st.add_n(269, len); st.add_n(270, ab);
        init();
    }
    __device__ __forceinline__ void add(uint32_t l, uint32_t a, uint32_t ct, Stats &st) {
        len += l; ab += a;
        const uint32_t sh = 16u * (ct & 1u);
        uint32_t &w = ct < 2 ? c01 : c23;
        w += 1u << sh;
        if (((w >> sh) & 0xffffu) == 0xffffu || len >= 0xf0000000u || ab >= 0xf0000000u) fold(st);
    }
};

template <int FAM>
struct Lane {
    Ep ep;
    PolAcc acc;
    PolMemo<FAM == 6 ? GF_MEMO6 : GF_MEMO4> pm;
    RelCache<FAM == 6 ? 10 : 4> rc;
    int added;
    LaneCnt sc;
    __device__ __forceinline__ void init() { ep.init(); acc.init(); pm.init(); rc.init(); added = 0; sc.init(); }
};
// Per-endpoint CT maps, non-strict accounting: the lane's net inserts belong to its
// current program's map, added to that map's count (no return value) when the lane
// moves to another program and at the end of the launch.
template <int FAM, bool PCT>
__device__ __forceinline__ void lane_flush_added(const IngCtx &X, Lane<FAM> &ln) {
    if constexpr (PCT) {
        if (ln.added && ln.ep.sl && !(X.strict & (FAM == 6 ? 2u : 1u)))
            atomicAdd(ing_ct<FAM, true>(X, ln.ep).count, (uint32_t)ln.added);
        ln.added = 0;
    }
}
// The lane's pending related-entry write (IPv4), to its map, and the cache dropped.
template <int FAM, bool PCT>
__device__ __forceinline__ void lane_rel_drop(const IngCtx &X, Lane<FAM> &ln) {
    if constexpr (PCT) {
        if (ln.ep.sl) rel_drop(ing_ct<FAM, true>(X, ln.ep), ln.rc, X.now);
        else ln.rc.slot = ~0u;                          // (nothing is pending before a program ran)
    } else {
        rel_drop(X.ct4, ln.rc, X.now);
    }
}

// handle_policy, bpf/bpf_lxc.c:980-1024.  FAM selects the CT path compiled in:
// 4 = the IPv4 path plus every packet that cannot reach conntrack (no IP
// header: their early returns need no CT code), 6 = IPv6 packets that reach
// conntrack.  The sort key keeps the two sets in different buckets.
template <int FAM, bool PCT, bool RL, bool DBG = false>
__device__ __forceinline__ gf_ingress_out handle_policy(const IngCtx &X, const gf_rec &r, uint32_t i, Lane<FAM> &ln,
                                                       uint32_t &ab, uint32_t *rlog, DbgLog *dl = nullptr) {
    gf_ingress_out o{};
    uint32_t sl = r.ep;
    if (!sl) { o.action = TC_SHOT; o.reason = 140; return o; }   // missed tail call (DROP_MISSED_TAIL_CALL)
    ln.ep.use(X, sl);
    uint32_t flags = ln.ep.flags;
    int fwd = 0, ret;
    uint8_t fl = 0;
    uint16_t proxy = 0;
    uint32_t ifindex = r.ifindex;
    uint32_t cls = r.cls & 3u;
    if (flags & GF_LXC_F_DROP_ALL) ret = D_POLICY;
    else if (cls == 2) {
        ab += 47;
        if constexpr (FAM == 6) ret = ipv6_policy<PCT, DBG>(X, ln.ep, r, i, fwd, fl, proxy, ifindex, &ln.added, ab, ln.acc, ln.rc, ln.pm, dl);
        else ret = D_INVALID;                       // ipv6_policy: short frame or batch without v6 columns
    }
    else if (cls == 1 && (flags & GF_LXC_F_LXC_IPV4)) {
        ab += 23;
        if constexpr (FAM == 4) ret = ipv4_policy<PCT, RL, DBG>(X, ln.ep, r, i, fwd, fl, proxy, ifindex, &ln.added, ab, ln.acc, ln.rc, ln.pm,
                                                  rlog, dl);
        else ret = D_INVALID;                       // (not reached: v4 packets sort into FAM 4 buckets)
    }
    else ret = D_UNKNOWN_L3;
    o.ct_ret = (uint8_t)fwd;
    if (ret < 0 || ret == TC_SHOT) {
        o.action = TC_SHOT; o.reason = (uint8_t)(-ret); o.flags = fl & GF_INGRESS_F_CREATED;
        return o;
    }
    o.flags = fl;
    o.proxy_port = proxy;
    o.ifindex_lo = (uint16_t)ifindex;
    o.action = ifindex ? TC_REDIRECT : TC_OK;
    return o;
}

// The 32-B record handle_policy reads and the packet's flow-group bucket key.
// Only packets that can reach conntrack (an IP header is present) are bound to
// their flow group; the rest carry no ordering constraint and are spread out.
// K.bits-1 bits of the group hash are the sort key (gf_key_bits): groups that collide
// share a bucket (always safe: a bucket is serialized as a whole), and a
// shorter key is one radix pass less.  The top key bit is the family of the CT
// path (1: IPv6 reaching conntrack).  skipped: a pipeline packet that ended
// before the cilium_policy tail call (cls bit 3; left untouched).
__device__ __forceinline__ uint32_t pack_rec(uint32_t i, uint32_t et, uint32_t len, uint32_t sa, uint32_t da,
                                             uint32_t w0, uint32_t w3, int l4, uint32_t proto, uint32_t sid,
                                             uint32_t ifx, uint16_t ep, uint32_t tci, bool skipped, bool have6,
                                             const uint32_t *s6, const uint32_t *d6, gf_rec &r,
                                             const gf_key_cfg &K) {
    r.len = len;
    r.saddr = sa; r.daddr = da;
    r.l4w0 = w0; r.l4w3 = (uint16_t)w3;
    r.src_identity = sid;
    r.ifindex = ifx;
    r.ep = ep;                                          // tail_call(cilium_policy, lxc_id) target
    r.l4_off = (int16_t)l4;
    r.proto = (uint8_t)proto;
    uint32_t cls = et == 0x0800 ? 1u : et == 0x86DD ? 2u : 0u;
    if (tci & 1) cls |= 4u;
    if (skipped) cls |= 8u;
    r.cls = (uint8_t)cls;
    if (skipped) return gf_key_skip(K);
    const bool ct_ok = ((cls & 3) == 1 && len >= 34) || ((cls & 3) == 2 && len >= 54 && have6);
    if (!ct_ok) return gf_key_live(gf_hash_words(&i, 1, 4), K);
    if ((cls & 3) == 2) return gf_key_live(gf_pair_hash6(s6, d6), K) | K.fam;
    return gf_key_live(gf_pair_hash4(sa, da), K);
}

__global__ __launch_bounds__(BLOCK) void k_ing_pack(gf_pkt_cols c, const uint16_t *slot_of, gf_rec *rec,
                                                    uint32_t *keys, gf_key_cfg K) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= c.n) return;
    const uint32_t et = c.ethertype[i], len = c.len[i];
    uint32_t s6[4] = {0, 0, 0, 0}, d6[4] = {0, 0, 0, 0};
    if (et == 0x86DD && len >= 54 && c.saddr6) {
        uint4 sv = reinterpret_cast<const uint4 *>(c.saddr6)[i];
        uint4 dv = gload<uint4>(c.daddr6 + 16 * (size_t)i);
        s6[0] = sv.x; s6[1] = sv.y; s6[2] = sv.z; s6[3] = sv.w;
        d6[0] = dv.x; d6[1] = dv.y; d6[2] = dv.z; d6[3] = dv.w;
    }
    gf_rec r;
    keys[i] = pack_rec(i, et, len, c.saddr4[i], c.daddr4[i], c.l4w0[i], c.l4w3[i], c.l4_off[i], c.proto[i],
                       c.src_identity ? c.src_identity[i] : 0u, c.ifindex ? c.ifindex[i] : 0u,
                       slot_of[c.lxc_id ? c.lxc_id[i] : 0], c.tc_index ? c.tc_index[i] : 0u, false,
                       c.saddr6 != nullptr, s6, d6, r, K);
    rec[i] = r;
}

// Flow-group schedule.  A bucket is a run of equal bucket keys (gf_key_cfg) in the
// stably sorted batch, so it holds whole flow groups with their packets in batch
// order.  One lane runs one bucket to completion, packet after packet — the
// order BPF would see them on one CPU — while different buckets (disjoint CT
// keys) run concurrently.  Buckets are handed out longest first
// (LPT): k_bucket_order lists them by packet count, descending, and waves take
// the next 64 entries of that list from a device queue, so the lanes of a wave
// carry equal work and the deepest buckets start first.
// The debug log entry of packet i: two 16-B stores, kept out of line (the IPv6
// kernel has no registers to spare for the inlined copy).
__device__ __attribute__((noinline)) void dbg_log_write_ol(uint4 *dlog, uint32_t i, DbgLog dl) {
    dlog[2 * (size_t)i] = make_uint4(dl.w[0], dl.w[1], dl.w[2], dl.w[3]);
    dlog[2 * (size_t)i + 1] = make_uint4(dl.w[4], dl.w[5], dl.w[6], dl.w[7]);
}
template <int FAM, bool PCT, bool RL, bool DBG = false>
__device__ __forceinline__ void ing_one(const IngCtx &X, uint32_t i, const gf_rec &r, gf_ingress_out *out,
                                        Stats &st, bool stats, Lane<FAM> &ln, uint32_t *rlog, uint4 *dlog = nullptr) {
    if (r.cls & 8) return;                              // pipeline: ended before the tail call
    uint32_t ab = 8;                                    // output record
    if constexpr (PCT) {
        // per-endpoint CT maps: the lane's related-entry cache belongs to its current
        // program's map; a packet of another program writes the pending entry first
        if (r.ep != ln.ep.sl) { lane_rel_drop<FAM, true>(X, ln); lane_flush_added<FAM, true>(X, ln); }
    }
    gf_ingress_out o;
    if constexpr (DBG) {
        // handle_policy with DEBUG: the log is written per packet, in bucket order, and only
        // for packets of a program with the flag (the others' entries stay cleared)
        DbgLog dl;
        dl.init();
        o = handle_policy<FAM, PCT, RL, true>(X, r, i, ln, ab, rlog, &dl);
        if (r.ep && (ln.ep.flags & GF_LXC_F_DEBUG)) dbg_log_write_ol(dlog, i, dl);
    } else {
        o = handle_policy<FAM, PCT, RL>(X, r, i, ln, ab, rlog);
    }
    if (X.pout && X.pout_wo) {                          // complete the pipeline record: stores only
        uint8_t *q = X.pout + 24 * (size_t)i;
        const uint32_t ff = ((uint32_t)(r.cls >> 4) & 7u) << 5;   // the front's whole GF_PIPE_F_* byte
        *reinterpret_cast<uint32_t *>(q) = GF_STAGE_POLICY | ((uint32_t)o.action << 8) | ((uint32_t)o.reason << 16) |
                                           ((uint32_t)o.ct_ret << 24);
        *reinterpret_cast<uint32_t *>(q + 4) = (ff | o.flags) | ((uint32_t)o.proxy_port << 16);
        *reinterpret_cast<uint16_t *>(q + 8) = o.ifindex_lo;
    } else if (X.pout) {                                // complete the pipeline / egress record
        uint8_t *q = X.pout + 24 * (size_t)i;
        uint2 a = *reinterpret_cast<const uint2 *>(q);
        uint2 b = *reinterpret_cast<const uint2 *>(q + 8);
        a.x = (a.x & 0xffu) | ((uint32_t)o.action << 8) | ((uint32_t)o.reason << 16) | ((uint32_t)o.ct_ret << 24);
        a.y = ((a.y & 0xffu) | o.flags) | (a.y & 0xff00u) | ((uint32_t)o.proxy_port << 16);
        b.x = (b.x & 0xffff0000u) | o.ifindex_lo;
        *reinterpret_cast<uint2 *>(q) = a;
        *reinterpret_cast<uint2 *>(q + 8) = b;
    } else {
        out[i] = o;
        GF_WR(WR_OUT);
    }
    if (stats) {
        st.add(o.reason); st.add(256 + o.action);
        ln.sc.add(r.len, ab, o.ct_ret & 3u, st);
    }
}

__device__ __forceinline__ gf_rec ld_rec(const gf_rec *rec, uint32_t i) { return rec[i]; }
__device__ __forceinline__ void flush_added(const IngCtx &X, uint32_t fam_bit, int added, uint32_t *ct_count,
                                            uint32_t *lds_added) {
    if (X.strict & fam_bit) return;
    if (added) atomicAdd(lds_added, (uint32_t)added);
    __syncthreads();
    if (threadIdx.x == 0 && *lds_added && ct_count) atomicAdd(ct_count, *lds_added);
}

// Bucket lists: one per family (IPv4 / IPv6 CT path), each the plain longest-first
// list.  (Lists per family x endpoint class, a workgroup starting on the class of
// the XCD it runs on so that an XCD's L2 would hold the policy maps of its class of
// endpoints only, measured slower with 8 classes: k_ing_groups 2.90 vs 2.40 ms on
// config 2, DESIGN.md.)
// Schedule words (device): hist[GF_FAMS][GF_LCAP+1] | base[..] | cursor[..] | nruns |
// queue[GF_FAMS] | nfam[GF_FAMS] | lcnt[GF_FAMS] | lstart[GF_FAMS] (family 0's list,
// then family 1's; each list by bucket size, descending).
#define GF_FAMS 2u            // families = lists: IPv4, IPv6
#define GF_LCAP 1024u
#define GF_SCHED_HIST(p) (p)
#define GF_SCHED_BASE(p) ((p) + GF_FAMS * (GF_LCAP + 1))
#define GF_SCHED_CURSOR(p) ((p) + 2 * GF_FAMS * (GF_LCAP + 1))
#define GF_SCHED_NRUNS(p) ((p) + 3 * GF_FAMS * (GF_LCAP + 1))
#define GF_SCHED_QUEUE(p) (GF_SCHED_NRUNS(p) + 1)
#define GF_SCHED_NFAM(p) (GF_SCHED_QUEUE(p) + GF_FAMS)
#define GF_SCHED_LCNT(p) (GF_SCHED_NFAM(p) + GF_FAMS)
#define GF_SCHED_LSTART(p) (GF_SCHED_LCNT(p) + GF_FAMS)
#define GF_SCHED_WORDS (3 * GF_FAMS * (GF_LCAP + 1) + 1 + 4 * GF_FAMS)
#define GF_SCHED_HBYTES (GF_FAMS * (GF_LCAP + 1) * 4)    // the block-local bins of k_bucket_hist / order (dynamic LDS)
// The list of a bucket: the family bit of its key.
__device__ __forceinline__ uint32_t sched_list(uint32_t key, const gf_key_cfg &K) { return key >> (K.bits - 1); }

// GRAB: buckets per lane per queue grab in the single-packet tail (GF_GRAB_ING for the
// egress deliveries' pass, whose buckets are mostly single packets; 1 elsewhere,
// where the extra state costs the kernel registers it cannot spare)
template <int FAM, int GRAB = 1, bool PCT = false, bool RL = false>
__global__ __launch_bounds__(BLOCK, FAM == 6 ? GF_ING_MINW6 : GF_ING_MINW) void k_ing_groups(IngCtx X, uint32_t *sched, const uint2 *order,
                                                      const uint32_t *perm,
                                                      const gf_rec *rec, gf_ingress_out *out, uint32_t *ct_count,
                                                      unsigned long long *stats) {
    constexpr int F = FAM == 6 ? 1 : 0;
    const uint32_t *nfam = GF_SCHED_NFAM(sched);
    if (nfam[F] == 0) return;                          // no bucket of this family (nothing to count either)
    __shared__ uint32_t sl[272];
    __shared__ uint32_t sadd;
    Stats st{sl};
    if (threadIdx.x == 0) sadd = 0;
    if (stats) st.init(); else __syncthreads();
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t *lcnt = GF_SCHED_LCNT(sched), *lstart = GF_SCHED_LSTART(sched);
    __shared__ Lane<FAM> lanes[BLOCK];
    Lane<FAM> &ln = lanes[threadIdx.x];
    ln.init();
    uint32_t *const rlog = RL && X.rlog && !(X.rlog_off && *X.rlog_off) ? X.rlog : nullptr;
    // (the family's one list.  The one-trip loop is what is left of a loop over several lists:
    // without it the compiler allocates this kernel's registers differently, which would have
    // to be measured again.)
    for (uint32_t li = 0; li < 1u; li++) {
    uint32_t *queue = GF_SCHED_QUEUE(sched) + F;
    const uint32_t nb = lcnt[F];
    const uint2 *lorder = order + lstart[F];
    // the wave's grab: [base, base + 64 * left) of the list, one 64-bucket round at a
    // time (wave-uniform values); grab = buckets per lane of the next grab
    uint32_t grab = 1, gbase = 0, left = 0;
    for (;;) {
        uint32_t t;
        bool first = false;
        if constexpr (GRAB == 1) {
            uint32_t base = 0;
            if (lane == 0) base = atomicAdd(queue, 64u);
            base = __shfl(base, 0);
            if (base >= nb) break;
            t = base + lane;
        } else {
            if (!left) {
                uint32_t b0 = 0;
                if (lane == 0) b0 = atomicAdd(queue, 64u * grab);
                gbase = (uint32_t)__builtin_amdgcn_readfirstlane((int)b0);
                left = grab;
            }
            if (gbase >= nb) break;
            t = gbase + lane;
            first = left == grab;
            gbase += 64u; left--;
        }
        if (t >= nb) continue;
        const uint2 oc = lorder[t];
        if (GRAB > 1 && first && (uint32_t)__builtin_amdgcn_readfirstlane((int)oc.y) == 1u) grab = GRAB;   // single-packet tail
        const uint32_t b = oc.x, c = oc.y;
        uint32_t i = perm[b];
        uint32_t inx = c > 1 ? perm[b + 1] : 0u;
        gf_rec r = ld_rec(rec, i);
        lane_rel_drop<FAM, PCT>(X, ln);                  // a new bucket: new flow groups
        uint4 pw = make_uint4(0, 0, 0, 0);               // perm[j & ~3 .. +3], j = b + k + 2: 16-B loads
        if (c > 2) pw = *reinterpret_cast<const uint4 *>(perm + ((b + 2) & ~3u));
        for (uint32_t k = 0; k < c; k++) {
            // the next record and the index after it are in flight while packet k runs
            uint32_t in2 = 0;
            if (k + 2 < c) {
                const uint32_t j = b + k + 2;
                if (!(j & 3u) && k) pw = *reinterpret_cast<const uint4 *>(perm + j);
                const uint32_t q = j & 3u;
                in2 = q == 0 ? pw.x : q == 1 ? pw.y : q == 2 ? pw.z : pw.w;
            }
            ing_one<FAM, PCT, RL>(X, i, r, out, st, stats != nullptr, ln, rlog);
            i = inx; inx = in2;
            if (k + 1 < c) r = ld_rec(rec, i);
        }
    }
    }
    ln.acc.flush(X);
    lane_rel_drop<FAM, PCT>(X, ln);                     // the pending related-entry write (IPv4)
    lane_flush_added<FAM, PCT>(X, ln);                  // (per-endpoint maps: the lane's own count add)
    if (stats) ln.sc.fold(st);
    flush_added(X, F ? 2u : 1u, ln.added, ct_count, &sadd);
    if (stats) st.flush(stats);
}

// The debug kernel (GF_LXC_F_DEBUG): k_ing_groups' schedule walk (one bucket per lane, GRAB 1, no
// related-entry log) over the debug instantiation of handle_policy, which also fills the
// per-packet log (dlog: a 32-B DbgLog per packet).  Launched by
// gf_policy_ingress_classify(_batches) only, when a ring is set and the array holds a program
// with the flag.  A copy of the loop, not a shared body: k_ing_groups keeps the code it had.
template <int FAM, bool PCT>
__global__ __launch_bounds__(BLOCK, FAM == 6 ? GF_ING_MINW6 : GF_ING_MINW) void k_ing_groups_dbg(IngCtx X, uint32_t *sched,
                                                      const uint2 *order, const uint32_t *perm,
                                                      const gf_rec *rec, gf_ingress_out *out, uint32_t *ct_count,
                                                      unsigned long long *stats, uint4 *dlog) {
    constexpr int F = FAM == 6 ? 1 : 0;
    if (GF_SCHED_NFAM(sched)[F] == 0) return;
    __shared__ uint32_t sl[272];
    __shared__ uint32_t sadd;
    Stats st{sl};
    if (threadIdx.x == 0) sadd = 0;
    if (stats) st.init(); else __syncthreads();
    const uint32_t lane = threadIdx.x & 63u;
    __shared__ Lane<FAM> lanes[BLOCK];
    Lane<FAM> &ln = lanes[threadIdx.x];
    ln.init();
    for (uint32_t li = 0; li < 1u; li++) {              // (one trip, as in k_ing_groups)
        uint32_t *queue = GF_SCHED_QUEUE(sched) + F;
        const uint32_t nb = GF_SCHED_LCNT(sched)[F];
        const uint2 *lorder = order + GF_SCHED_LSTART(sched)[F];
        for (;;) {
            uint32_t base = 0;
            if (lane == 0) base = atomicAdd(queue, 64u);
            base = __shfl(base, 0);
            if (base >= nb) break;
            const uint32_t t = base + lane;
            if (t >= nb) continue;
            const uint2 oc = lorder[t];
            lane_rel_drop<FAM, PCT>(X, ln);              // a new bucket: new flow groups
            for (uint32_t k = 0; k < oc.y; k++) {        // the bucket's packets in batch order
                const uint32_t i = perm[oc.x + k];
                ing_one<FAM, PCT, false, true>(X, i, ld_rec(rec, i), out, st, stats != nullptr, ln, nullptr, dlog);
            }
        }
    }
    ln.acc.flush(X);
    lane_rel_drop<FAM, PCT>(X, ln);
    lane_flush_added<FAM, PCT>(X, ln);
    if (stats) ln.sc.fold(st);
    flush_added(X, F ? 2u : 1u, ln.added, ct_count, &sadd);
    if (stats) st.flush(stats);
}

// ---- programs without conntrack (GF_LXC_F_NO_CONNTRACK: CONNTRACK undefined) ----
// bpf/lib/conntrack.h:582-617: ct_lookup4/6 return 0 (CT_NEW) and touch neither a
// map nor the tuple, ct_create4/6 return 0, ct_delete4/6 are empty.  What is left of
// ipv4_policy / ipv6_policy (bpf_lxc.c:865-970, 745-862): the tuple keeps the frame's
// addresses unreversed and ports / flags 0, no L4 header byte is read, the policy is
// asked with dport 0 and every packet a rule does not allow is DROP_POLICY (nothing
// is a reply or related).  A packet reads no CT line and is ordered against no
// other packet, so these packets take no part in the flow-group schedule: one thread
// per packet in batch order (k_ing_noct).
// policy_can_access_ingress with the counter update, the entry counted at once
// (policy.h:67-92; counter sums commute).
__device__ __forceinline__ int policy_ingress_noct(const IngCtx &X, const Ep &ep, uint32_t identity, uint32_t proto,
                                                   uint32_t len, bool v6, const uint32_t *cidr_addr, uint32_t &ab) {
    PolLine pl;
    int64_t fc;
    const int v = policy_lookup(X, ep, pl, false, identity, 0u, proto, v6, cidr_addr, ab, fc);
    if (fc >= 0) pol_count_add(ep.pol_side + (uint64_t)fc * GF_POL_SIDE, 1u, len, false);
    return v;
}
// ipv{4,6}_redirect_to_host_port of a verdict > 0 (ret == CT_NEW always holds): the
// proxy-map key and the port rewrite come from the unfilled tuple (sport and the old
// dport 0, key .saddr = the frame's daddr)
__device__ __forceinline__ int redirect_noct(const IngCtx &X, const gf_rec &r, uint32_t i, int verdict, V6Tuple tv,
                                             bool v6, uint4 od, uint8_t &ofl, uint16_t &proxy, uint32_t &ifindex) {
    if (X.tmark)
        trace_proxy(X.tmark, X.tcap, X.snap ? X.snap + (size_t)i * X.snap_stride : nullptr, nullptr, 0,
                    trace_cap_len(r.len, X.snap_stride), i, GF_TR_PX_POLICY);
    const int r3 = redirect_checks(r.len, r.l4_off, r.proto);
    if (r3 < 0) return r3;
    if (X.snap || X.plog) {
        if (v6) pol_redirect_ol(pol_ctx(X), i, r.len, r.l4_off, r.proto, tv, (uint32_t)verdict & 0xffffu, od, r.src_identity);
        else { const uint32_t odw[1] = {od.x}; pol_redirect(X, i, r.len, r.l4_off, r.proto, tv.w, false, (uint32_t)verdict & 0xffffu, odw, r.src_identity); }
    }
    ifindex = X.host_ifindex;
    ofl |= GF_INGRESS_F_PROXY;
    proxy = (uint16_t)verdict;
    return 0;
}
// handle_policy (bpf_lxc.c:980-1024) of a program without conntrack
__device__ __forceinline__ gf_ingress_out handle_policy_noct(const IngCtx &X, const gf_rec &r, uint32_t i, uint32_t &ab) {
    gf_ingress_out o{};
    if (!r.ep) { o.action = TC_SHOT; o.reason = 140; return o; }   // missed tail call (DROP_MISSED_TAIL_CALL)
    Ep ep;
    ep.init();
    ep.use(X, r.ep);
    const uint32_t flags = ep.flags, len = r.len, nh = r.proto, cls = r.cls & 3u;
    int ret;
    uint8_t fl = 0;
    uint16_t proxy = 0;
    uint32_t ifindex = r.ifindex;
    if (flags & GF_LXC_F_DROP_ALL) ret = D_POLICY;
    else if (cls == 2) {                                // ipv6_policy
        ab += 47;
        if (len < 54 || !X.daddr6 || !X.saddr6) ret = D_INVALID;
        else {
            const uint4 d = gload<uint4>(X.daddr6 + (size_t)X.a6_stride * i);
            const uint4 s = gload<uint4>(X.saddr6 + (size_t)X.a6_stride * i);
            const uint32_t co = csum_l4_offset(nh), rn_new = d.w & 0xffffu;   // the rev-NAT index in the address (:776-790)
            ret = 0;
            if (rn_new) {
                if (X.snap) pol_v6_zero_rn_ol(pol_ctx(X), i, len, r.l4_off, nh, rn_new);
                if (co && !l4csum_ok(r.l4_off + (int)co, len)) ret = D_CSUM_L4;
            }
            if (!ret) {
                const uint32_t sa[4] = {s.x, s.y, s.z, s.w};
                int verdict = policy_ingress_noct(X, ep, r.src_identity, nh, len, true, sa, ab);
                if (verdict < 0) ret = D_POLICY;
                else {
                    if (r.cls & 4) verdict = 0;         // skip_proxy
                    if (verdict > 0) {
                        V6Tuple tv{{d.x, d.y, d.z, d.w, s.x, s.y, s.z, s.w, 0u, nh}};
                        ret = redirect_noct(X, r, i, verdict, tv, true, d, fl, proxy, ifindex);
                    }
                }
            }
        }
    }
    else if (cls == 1 && (flags & GF_LXC_F_LXC_IPV4)) { // ipv4_policy
        ab += 23;
        if (len < 34) ret = D_INVALID;
        else {
            const uint32_t sa[1] = {r.saddr};
            int verdict = policy_ingress_noct(X, ep, r.src_identity, nh, len, false, sa, ab);
            ret = 0;
            if (verdict < 0) ret = D_POLICY;
            else {
                if (r.cls & 4) verdict = 0;
                if (verdict > 0) {
                    V6Tuple tv{{r.daddr, r.saddr, 0u, nh, 0u, 0u, 0u, 0u, 0u, 0u}};
                    ret = redirect_noct(X, r, i, verdict, tv, false, make_uint4(r.daddr, 0u, 0u, 0u), fl, proxy, ifindex);
                }
            }
        }
    }
    else ret = D_UNKNOWN_L3;
    if (ret < 0) { o.action = TC_SHOT; o.reason = (uint8_t)(-ret); return o; }
    o.flags = fl;
    o.proxy_port = proxy;
    o.ifindex_lo = (uint16_t)ifindex;
    o.action = ifindex ? TC_REDIRECT : TC_OK;
    return o;
}
// A mixed array: the packets of programs without conntrack leave the flow-group
// sort's live range (the grouped kernels never see them).
__global__ __launch_bounds__(BLOCK) void k_ing_noct_mark(uint32_t n, const gf_rec *rec, const gf_lxc_dev *cfgs,
                                                         uint32_t *keys, gf_key_cfg K) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t ep = rec[i].ep;
    if (ep && (cfgs[ep - 1].flags & GF_LXC_F_NO_CONNTRACK)) keys[i] = gf_key_skip(K);
}
// A HASH CT map that could fill during the batch makes every insert of its family
// order-dependent (E2BIG for whichever comes last): the family's packets become one
// bucket, which one lane runs in batch order (fams bit 0: the IPv4 list, which also
// holds the packets that reach no conntrack; bit 1: IPv6).  Skipped packets stay out.
__global__ __launch_bounds__(BLOCK) void k_ing_serial_keys(uint32_t n, uint32_t *keys, gf_key_cfg K, uint32_t fams) {
    for (uint32_t i = blockIdx.x * BLOCK + threadIdx.x; i < n; i += gridDim.x * BLOCK) {
        const uint32_t k = keys[i];
        if (k == gf_key_skip(K)) continue;
        if (fams & ((k & K.fam) ? 2u : 1u)) keys[i] = k & K.fam;
    }
}
// One thread per packet in batch order: coalesced record reads and out[i] (or pipeline
// record, X.pout) writes, the
// block's counter bins in LDS, policy counters by atomics, no lane state.
// all: every program of the array is without conntrack (the kernel then also reports
// the packets of empty slots); else it runs exactly the packets k_ing_noct_mark took
// out of the schedule.
__global__ __launch_bounds__(BLOCK) void k_ing_noct(IngCtx X, uint32_t n, uint32_t all, const gf_rec *rec,
                                                    gf_ingress_out *out, unsigned long long *stats) {
    __shared__ uint32_t sl[272];
    Stats st{sl};
    if (stats) st.init();
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    bool act = false;
    gf_ingress_out o{};
    uint32_t len = 0, ab = 0;
    if (i < n) {
        const gf_rec r = rec[i];
        act = !(r.cls & 8) && (all || (r.ep && (gload<uint32_t>(&X.cfgs[r.ep - 1].flags) & GF_LXC_F_NO_CONNTRACK)));
        if (act) {
            len = r.len; ab = 8;                        // output record
            o = handle_policy_noct(X, r, i, ab);
            if (X.pout && X.pout_wo) {                  // complete the pipeline record: stores only (as ing_one)
                uint8_t *q = X.pout + 24 * (size_t)i;
                const uint32_t ff = ((uint32_t)(r.cls >> 4) & 7u) << 5;   // the front's whole GF_PIPE_F_* byte
                *reinterpret_cast<uint32_t *>(q) = GF_STAGE_POLICY | ((uint32_t)o.action << 8) | ((uint32_t)o.reason << 16) |
                                                   ((uint32_t)o.ct_ret << 24);
                *reinterpret_cast<uint32_t *>(q + 4) = (ff | o.flags) | ((uint32_t)o.proxy_port << 16);
                *reinterpret_cast<uint16_t *>(q + 8) = o.ifindex_lo;
            } else if (X.pout) {                        // a record whose other bytes are kept
                uint8_t *q = X.pout + 24 * (size_t)i;
                uint2 a = *reinterpret_cast<const uint2 *>(q);
                uint2 b = *reinterpret_cast<const uint2 *>(q + 8);
                a.x = (a.x & 0xffu) | ((uint32_t)o.action << 8) | ((uint32_t)o.reason << 16) | ((uint32_t)o.ct_ret << 24);
                a.y = ((a.y & 0xffu) | o.flags) | (a.y & 0xff00u) | ((uint32_t)o.proxy_port << 16);
                b.x = (b.x & 0xffff0000u) | o.ifindex_lo;
                *reinterpret_cast<uint2 *>(q) = a;
                *reinterpret_cast<uint2 *>(q + 8) = b;
            } else {
                out[i] = o;
            }
        }
    }
    if (stats) {                                        // (every lane: wave sums; all CT_NEW)
        st.pkt_wave(act, o.reason, o.action, len, ab);
        const uint32_t c = (uint32_t)__popcll(__ballot(act));
        if ((threadIdx.x & 63u) == 0) st.add_n(264, c);
        st.flush(stats);
    }
}

// Bucket-size histogram per family (the top bit of the bucket's sorted key, K.fam):
// block-local LDS bins, one global add per non-empty bin.
#define GF_SCHED_ITEMS 4096
// off[q]: the start of run q in the sorted keys (nruns of them); its length is
// the distance to the next start (or to n).  (rec and perm are not read: they gave a
// bucket's endpoint class when the lists had classes, and stay in the two signatures so
// that the kernels compile to the code they were measured as.)
__global__ __launch_bounds__(BLOCK) void k_bucket_hist(uint32_t n, const uint32_t *off, const uint32_t *skeys,
                                                       const gf_rec *rec, const uint32_t *perm, uint32_t *sched,
                                                       gf_key_cfg K) {
    extern __shared__ uint32_t h[];                     // GF_SCHED_HBYTES
    for (uint32_t k = threadIdx.x; k < GF_FAMS * (GF_LCAP + 1); k += blockDim.x) h[k] = 0;
    __syncthreads();
    uint32_t nq = *GF_SCHED_NRUNS(sched);
    uint32_t b0 = blockIdx.x * GF_SCHED_ITEMS;
    for (uint32_t q = b0 + threadIdx.x; q < b0 + GF_SCHED_ITEMS && q < nq; q += blockDim.x) {
        const uint32_t key = skeys[off[q]];
        uint32_t c = (q + 1 < nq ? off[q + 1] : n) - off[q];
        if (c && key != gf_key_skip(K))
            atomicAdd(&h[sched_list(key, K) * (GF_LCAP + 1) + (c < GF_LCAP ? c : GF_LCAP)], 1u);
    }
    __syncthreads();
    uint32_t *hist = GF_SCHED_HIST(sched);
    for (uint32_t k = threadIdx.x; k < GF_FAMS * (GF_LCAP + 1); k += blockDim.x)
        if (h[k]) atomicAdd(&hist[k], h[k]);
}

// base[l][c] = start of (list l, count c) in the order array: the lists one after
// the other, each by count descending.  One block of GF_LCAP threads (thread k owns
// bin c = GF_LCAP - k); also clears the cursors and the work queues and writes each
// list's count and start and each family's total.
__global__ __launch_bounds__(GF_LCAP) void k_bucket_base(uint32_t *sched) {
    __shared__ uint32_t s[GF_LCAP];
    __shared__ uint32_t tot;
    const uint32_t k = threadIdx.x, c = GF_LCAP - k;
    const uint32_t *hist = GF_SCHED_HIST(sched);
    uint32_t *base = GF_SCHED_BASE(sched), *cursor = GF_SCHED_CURSOR(sched);
    if (k == 0) { tot = 0; GF_SCHED_NFAM(sched)[0] = GF_SCHED_NFAM(sched)[1] = 0; }
    __syncthreads();
    for (uint32_t l = 0; l < GF_FAMS; l++) {
        const uint32_t *hf = hist + l * (GF_LCAP + 1);
        s[k] = hf[c];
        __syncthreads();
        for (uint32_t d = 1; d < GF_LCAP; d <<= 1) {    // inclusive scan over bins GF_LCAP .. 1
            uint32_t v = k >= d ? s[k - d] : 0u;
            __syncthreads();
            s[k] += v;
            __syncthreads();
        }
        const uint32_t add = tot;
        base[l * (GF_LCAP + 1) + c] = add + s[k] - hf[c];
        cursor[l * (GF_LCAP + 1) + c] = 0;
        if (k == 0) { base[l * (GF_LCAP + 1)] = add; cursor[l * (GF_LCAP + 1)] = 0; }
        __syncthreads();
        if (k == GF_LCAP - 1) {
            GF_SCHED_LCNT(sched)[l] = s[k];
            GF_SCHED_LSTART(sched)[l] = add;
            GF_SCHED_NFAM(sched)[l] += s[k];
            GF_SCHED_QUEUE(sched)[l] = 0;
            tot = add + s[k];
        }
        __syncthreads();
    }
}

// order[] = {first sorted position, packet count} of the non-empty buckets,
// family 0 then 1, each by count descending (ties in any order): block-local
// counts per bin, one global reservation per (block, bin).
__global__ __launch_bounds__(BLOCK) void k_bucket_order(uint32_t n, const uint32_t *off, const uint32_t *skeys,
                                                        const gf_rec *rec, const uint32_t *perm, uint32_t *sched,
                                                        uint2 *order, uint32_t skip1, gf_key_cfg K) {
    extern __shared__ uint32_t h[];                     // GF_SCHED_HBYTES
    for (uint32_t k = threadIdx.x; k < GF_FAMS * (GF_LCAP + 1); k += blockDim.x) h[k] = 0;
    __syncthreads();
    uint32_t nq = *GF_SCHED_NRUNS(sched);
    const uint32_t *base = GF_SCHED_BASE(sched);
    uint32_t *cursor = GF_SCHED_CURSOR(sched);
    uint32_t b0 = blockIdx.x * GF_SCHED_ITEMS;
    for (uint32_t q = b0 + threadIdx.x; q < b0 + GF_SCHED_ITEMS && q < nq; q += blockDim.x) {
        const uint32_t key = skeys[off[q]];
        uint32_t c = (q + 1 < nq ? off[q + 1] : n) - off[q];
        if (c && key != gf_key_skip(K) && !(skip1 && c == 1))
            atomicAdd(&h[sched_list(key, K) * (GF_LCAP + 1) + (c < GF_LCAP ? c : GF_LCAP)], 1u);
    }
    __syncthreads();
    for (uint32_t k = threadIdx.x; k < GF_FAMS * (GF_LCAP + 1); k += blockDim.x)
        if (h[k]) h[k] = base[k] + atomicAdd(&cursor[k], h[k]);
    __syncthreads();
    for (uint32_t q = b0 + threadIdx.x; q < b0 + GF_SCHED_ITEMS && q < nq; q += blockDim.x) {
        const uint32_t key = skeys[off[q]];
        uint32_t c = (q + 1 < nq ? off[q + 1] : n) - off[q];
        if (c && key != gf_key_skip(K) && !(skip1 && c == 1))
            order[atomicAdd(&h[sched_list(key, K) * (GF_LCAP + 1) + (c < GF_LCAP ? c : GF_LCAP)], 1u)] =
                make_uint2(off[q], c);
    }
}
// Single-packet buckets in packet-index order (the egress passes,
// whose connection groups are mostly one packet a step): the tail of each family's
// list (bin c = 1) is filled by packet index, so a wave's lanes read neighbouring
// records, frames and output rows instead of 64 random ones.  k_single_mark writes
// each such packet's word sw[i] = (bucket start + 1) << 1 | family (one 4-B store;
// 0 = not a single-packet bucket); k_single_count / k_run_scan / k_single_write
// rank them per family in index order.
__global__ __launch_bounds__(BLOCK) void k_single_mark(uint32_t n, const uint32_t *off, const uint32_t *skeys,
                                                       const uint32_t *perm, const uint32_t *sched, uint32_t *sw,
                                                       gf_key_cfg K) {
    const uint32_t nq = *GF_SCHED_NRUNS(sched);
    for (uint32_t q = blockIdx.x * BLOCK + threadIdx.x; q < nq; q += gridDim.x * BLOCK) {
        const uint32_t b = off[q], key = skeys[b];
        if ((q + 1 < nq ? off[q + 1] : n) - b != 1u || key == gf_key_skip(K)) continue;
        sw[perm[b]] = ((b + 1u) << 1) | (key >> (K.bits - 1));
    }
}
// the family of a packet's single-bucket word: 1 / 2, 0 = none
__device__ __forceinline__ uint32_t single_fam(uint32_t w) { return w ? 1u + (w & 1u) : 0u; }
__global__ __launch_bounds__(BLOCK) void k_single_count(uint32_t n, const uint32_t *sw, uint32_t *t0, uint32_t *t1) {
    __shared__ uint32_t wc[2][BLOCK / 64];
    const uint32_t b0 = blockIdx.x * GF_RUN_ITEMS, lane = threadIdx.x & 63u;
    uint32_t c0 = 0, c1 = 0;
    for (uint32_t k = 0; k < GF_RUN_ITEMS / BLOCK; k++) {
        const uint32_t j = b0 + k * BLOCK + threadIdx.x;
        const uint32_t f = j < n ? single_fam(sw[j]) : 0u;
        c0 += (uint32_t)__popcll(__ballot(f == 1u));
        c1 += (uint32_t)__popcll(__ballot(f == 2u));
    }
    if (lane == 0) { wc[0][threadIdx.x >> 6] = c0; wc[1][threadIdx.x >> 6] = c1; }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t a = 0, z = 0;
        for (uint32_t w = 0; w < BLOCK / 64; w++) { a += wc[0][w]; z += wc[1][w]; }
        t0[blockIdx.x] = a; t1[blockIdx.x] = z;
    }
}
__global__ __launch_bounds__(BLOCK) void k_single_write(uint32_t n, const uint32_t *sw, const uint32_t *t0,
                                                        const uint32_t *t1, const uint32_t *sched, uint2 *order) {
    __shared__ uint32_t wc[2][BLOCK / 64];
    const uint32_t b0 = blockIdx.x * GF_RUN_ITEMS, lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const uint32_t *base = GF_SCHED_BASE(sched);         // bin c = 1 of family f's list
    uint32_t p0 = base[0 * (GF_LCAP + 1) + 1] + t0[blockIdx.x], p1 = base[1 * (GF_LCAP + 1) + 1] + t1[blockIdx.x];
    for (uint32_t k = 0; k < GF_RUN_ITEMS / BLOCK; k++) {
        const uint32_t j = b0 + k * BLOCK + threadIdx.x;
        const uint32_t w = j < n ? sw[j] : 0u, f = single_fam(w);
        const uint64_t m0 = __ballot(f == 1u), m1 = __ballot(f == 2u);
        if (lane == 0) { wc[0][wv] = (uint32_t)__popcll(m0); wc[1][wv] = (uint32_t)__popcll(m1); }
        __syncthreads();
        uint32_t e0 = 0, e1 = 0, a0 = 0, a1 = 0;
        for (uint32_t q = 0; q < BLOCK / 64; q++) {
            e0 += q < wv ? wc[0][q] : 0u; e1 += q < wv ? wc[1][q] : 0u;
            a0 += wc[0][q]; a1 += wc[1][q];
        }
        const uint64_t below = (1ull << lane) - 1ull;
        if (f == 1u) order[p0 + e0 + (uint32_t)__popcll(m0 & below)] = make_uint2((w >> 1) - 1u, 1u);
        if (f == 2u) order[p1 + e1 + (uint32_t)__popcll(m1 & below)] = make_uint2((w >> 1) - 1u, 1u);
        p0 += a0; p1 += a1;
        __syncthreads();
    }
}

// ================================================================ pipeline (config 4)
// bpf_xdp -> bpf_lb from-netdev -> bpf_netdev from-netdev -> cilium_policy tail
// call, each program seeing the frame as the previous one rewrote it.
// k_pipe_front stages a block's frames in LDS and runs the first three on one
// packet per lane over its frame there (the rewrites and their checksum updates
// are applied to that copy), re-parses the rewritten header and writes the
// packet's handle_policy record and flow-group key directly (k_ing_pack fused);
// the ingress machinery then runs handle_policy on the packets that reached the
// tail call and completes their pipeline records in place.
// k_nd_front (a netdev stage with HANDLE_NS or ENCAP_IFINDEX), k_ovl_front (from-overlay)
// and k_host_front (from-host) are the other frame entry points.  All four are front_body
// around the entry's own programs: the tile, the record hand-off to ingress_run and the
// counters exist once.

// cilium_lxc as the entry programs look it up
struct LxcDev {
    gf_htab_desc lxc;
    const uint32_t *lxset;         // cilium_lxc's IPv4 keys: address set + slots (Map::addr_set), or null
    uint32_t lxbits, lxzero;
};
// What the ENCAP_IFINDEX branches read (host_encap4 / 6): the node's tunnel map and cluster range
struct EncapDev {
    gf_htab_desc tunnel;
    const uint32_t *tnset;         // the tunnel map's IPv4 keys (Map::addr_set), or null
    uint32_t tnbits, tnzero;
    uint32_t encap_ifindex, cluster_range, cluster_mask, ipv4_mask;
    uint32_t node6[3];             // first 12 bytes of gf_node_cfg.router_ip6 (ipv6_match_prefix_96)
};
struct NetdevDev {
    LxcDev lx;
    uint32_t flags, fixed_secctx;
    uint32_t router6[2];           // first 8 bytes of ROUTER_IP (LE words)
};
struct PipeDev {
    XdpDev x;
    LbDev L;
    NetdevDev nd;
    uint32_t has_xdp, has_lb, lb_redirect_ifindex, vec_copy;
    uint8_t *tcap_in;              // TRACE_FROM_STACK captures (128 B per packet; null: the netdev does not trace)
};
// The netdev stage's options (k_nd_front only): from_netdev as bpf/init.sh builds it for the
// native device (:179 -DHANDLE_NS; ENCAP_IFINDEX from node_config.h in tunnel mode, :303-304)
struct NdxDev {
    EncapDev enc;
    uint32_t router6[4];           // ROUTER_IP (gf_netdev_cfg.router_ip6): icmp6_handle's echo test
    uint32_t *tunnel_ip;           // bpf_tunnel_key.remote_ipv4 per frame (0: no encap), or null
};

// One lane's packet on its way through a front kernel: its row in LDS, the header as received,
// what the entry's programs found out, and the record they fill.
struct FrontLane {
    uint32_t i, len, et;
    Row w;
    PktHdr h;
    gf_pipeline_out o;
    uint32_t sec, ifx, lxc;        // the source identity; cb[CB_IFINDEX] and the lxc_id of the tail call
    uint32_t mapped, ndport;       // map_lxc_in rewrote the dport
    uint32_t tun_ip, call, rev;    // encap's remote_ipv4; the responder call; reverse_proxy translated
    uint32_t ab;                   // algorithmic bytes so far
    uint32_t tci_or;               // ORed into tc_index for handle_policy
    bool tail;                     // reached tail_call(cilium_policy)
    bool keep_sec;                 // not tail: sec stays in the skipped record (an encap redirect:
                                   // TRACE_TO_OVERLAY's label)
};
// lb4_xlate / lb6_xlate writes (bpf/lib/lb.h:615-659, 397-423) of a translation
// lb_v4/lb_v6 accepted (their checks passed, so every helper succeeds).
__device__ void pipe_lb_rewrite(Row &w, uint32_t len, const PktHdr &h, bool v6, const gf_lb_out &o,
                                const uint32_t *n6, uint32_t key_dport, uint32_t &ab) {
    const uint32_t nh = h.proto;
    const int l4_off = h.l4;
    uint32_t sum = 0;
    if (!v6) {
        const uint32_t old = h.da, nw = o.new_daddr4;
        w.w32(30, nw);
        sum = ck_add(ck_add(0u, ~old), nw);             // csum_diff(&key->address, 4, new_daddr, 4, 0)
        l3_csum(w, len, 24, 0, sum, 0);
        ab += 4 + 2;
    } else {
        const uint32_t *od = h.d6;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            w.w32(38 + 4 * k, n6[k]);                   // ipv6_store_daddr
            sum = ck_add(ck_add(sum, ~od[k]), n6[k]);
        }
        ab += 16;
    }
    const uint32_t co = csum_l4_offset(nh), fl = nh == 17 ? GF_F_MANGLED_0 : 0u;
    if (co || v6) { l4_csum(w, len, l4_off + (int)co, 0, sum, GF_F_PSEUDO_HDR | fl); ab += 2; }
    if (o.new_dport) {                                  // l4_modify_port, bpf/lib/l4.h:50-60
        l4_csum(w, len, l4_off + (int)co, key_dport, o.new_dport, 2u | fl);
        w.w16((uint32_t)(l4_off + 2), o.new_dport);
        ab += 4;
    }
}

enum { ND_TAILCALL = 1000, ND_ICMP6_TE = 1001 };

// The common tail of ipv{4,6}_local_delivery (bpf/lib/l3.h:106-168): MACs,
// map_lxc_in (l3.h:71-104 + l4_port_map_in, bpf/lib/l4.h:62-88: every portmap
// entry is compared with the dport loaded once), cb[], tail call.
__device__ int delivery_tail(Row &w, uint32_t len, int l4_off, uint32_t nh, const uint8_t *ep, uint32_t &ifx,
                             uint32_t &lxc, uint32_t &mapped, uint32_t &ndport, uint32_t &ab) {
    const uint32_t m0 = gload<uint32_t>(ep + 16), m1 = gload<uint32_t>(ep + 20);
    const uint32_t r0 = gload<uint32_t>(ep + 24), r1 = gload<uint32_t>(ep + 28);
    w.w32(6, r0); w.w16(10, r1 & 0xffffu);              // eth_store_saddr(node_mac)
    w.w32(0, m0); w.w16(4, m1 & 0xffffu);               // eth_store_daddr(mac)
    ab += 16 + 12;
    const uint32_t pm0 = gload<uint32_t>(ep + 48);
    ab += 4;
    if ((pm0 >> 16) && (nh == 6 || nh == 17)) {
        if (!skb_ok(l4_off + 2, 2, len)) return D_INVALID;
        const uint32_t dport = w.r16((uint32_t)(l4_off + 2));
        const uint32_t co = csum_l4_offset(nh), fl = nh == 17 ? GF_F_MANGLED_0 : 0u;
        for (int k = 0; k < 16; k++) {                  // PORTMAP_MAX
            const uint32_t pm = k ? gload<uint32_t>(ep + 48 + 4 * k) : pm0;
            const uint32_t from = pm & 0xffffu, to = pm >> 16;
            if (k) ab += 4;
            if (!to || !from) break;
            if (from != dport) continue;
            if (l4_csum(w, len, l4_off + (int)co, dport, to, 2u | fl) < 0) return D_CSUM_L4;
            if (!skb_ok(l4_off + 2, 2, len)) return D_WRITE_ERROR;
            w.w16((uint32_t)(l4_off + 2), to);
            mapped = 1; ndport = to;
            ab += 4;
        }
    }
    ifx = gload<uint32_t>(ep);                          // cb[CB_IFINDEX] = ep->ifindex
    lxc = gload<uint16_t>(ep + 6);                      // tail_call(cilium_policy, ep->lxc_id)
    return ND_TAILCALL;
}

// ---- pieces the entry programs share
// lookup_ip4_endpoint / lookup_ip6_endpoint: the endpoint's cilium_lxc value, or null
__device__ __forceinline__ const uint8_t *lxc_lookup4(const LxcDev &X, uint32_t da, uint32_t &ab) {
    uint32_t kw[5] = {da, 0, 0, 0, 1u};
    const int64_t f = X.lxset ? aset_slot(X.lxset, X.lxbits, X.lxzero, kw[0]) : ht_find<20>(X.lxc, kw, key_hash<20>(kw));
    ab += 20;
    if (f < 0) return nullptr;
    ab += 8;
    return ht_val(X.lxc, f);
}
__device__ __forceinline__ const uint8_t *lxc_lookup6(const LxcDev &X, const Row &w, uint32_t &ab) {
    uint32_t kw[5] = {w.r32(38), w.r32(42), w.r32(46), w.r32(50), 2u};
    const int64_t f = ht_find<20>(X.lxc, kw, key_hash<20>(kw));
    ab += 20 + 8;
    if (f < 0) return nullptr;
    ab += 8;
    return ht_val(X.lxc, f);
}
__device__ __forceinline__ bool ep_is_host(const uint8_t *ep) { return gload<uint32_t>(ep + 8) & 1u; }   // ENDPOINT_F_HOST

// ipv4_dec_ttl (bpf/lib/ipv4.h:30-43) / ipv6_dec_hoplimit (bpf/lib/ipv6.h:178-193): 0, or what
// the program returns instead of going on
__device__ __forceinline__ int dec_ttl4(FrontLane &L) {
    const uint32_t ttl = L.w.b(22);
    if (ttl <= 1) return D_INVALID;
    l3_csum(L.w, L.len, 24, ttl, ttl - 1, 2);
    L.w.w8(22, ttl - 1);
    L.ab += 3;
    return 0;
}
__device__ __forceinline__ int dec_hoplimit6(FrontLane &L) {
    const uint32_t hl = L.w.b(21);
    if (hl <= 1) return ND_ICMP6_TE;
    L.w.w8(21, hl - 1);
    L.ab += 1;
    return 0;
}
// ipv4_local_delivery / ipv6_local_delivery (bpf/lib/l3.h:106-168)
__device__ __forceinline__ int local_delivery4(FrontLane &L, const uint8_t *ep) {
    if (const int e = dec_ttl4(L)) return e;
    return delivery_tail(L.w, L.len, L.h.l4, L.h.proto, ep, L.ifx, L.lxc, L.mapped, L.ndport, L.ab);
}
__device__ __forceinline__ int local_delivery6(FrontLane &L, const uint8_t *ep) {
    if (const int e = dec_hoplimit6(L)) return e;
    return delivery_tail(L.w, L.len, L.h.l4, L.h.proto, ep, L.ifx, L.lxc, L.mapped, L.ndport, L.ab);
}

// derive_sec_ctx (bpf_netdev.c:50-64) of an IPv6 frame; flags: GF_NETDEV_F_*, router6: the first
// 8 bytes of ROUTER_IP
__device__ __forceinline__ uint32_t derive_sec_ctx6(const Row &w, uint32_t flags, uint32_t fixed_secctx,
                                                    const uint32_t *router6) {
    if (flags & GF_NETDEV_F_FIXED_SECCTX) return fixed_secctx;
    if (w.r32(22) == router6[0] && w.r32(26) == router6[1])
        return __builtin_bswap32(w.r32(14) & __builtin_bswap32(0x000FFFFFu));
    return 2u;                                          // WORLD_ID
}

// The ENCAP_IFINDEX branch of handle_ipv4 (:378-393) / handle_ipv6 (:225-243) once the
// endpoint lookup missed: the cluster-range test and encap_and_redirect's tunnel-map lookup
// (lib/encap.h:30-70).  true: tun_ip = bpf_tunnel_key.remote_ipv4; false: not in the range, or
// DROP_NO_TUNNEL_ENDPOINT, which both callers turn into TC_ACT_OK.
enum { HO_ENCAP = 1003 };
__device__ __forceinline__ bool host_encap4(const EncapDev &H, uint32_t da, uint32_t &tun_ip, uint32_t &ab) {
    if (H.encap_ifindex && (da & H.cluster_mask) == H.cluster_range) {
        uint32_t tk[5] = {da & H.ipv4_mask, 0, 0, 0, 1u};
        const int64_t ft = H.tnset ? aset_slot(H.tnset, H.tnbits, H.tnzero, tk[0]) : ht_find<20>(H.tunnel, tk, key_hash<20>(tk));
        ab += 20;
        if (ft >= 0) {                                  // encap_and_redirect (lib/encap.h:30-70)
            tun_ip = __builtin_bswap32(gload<uint32_t>(ht_val(H.tunnel, ft)));
            ab += 20;
            return true;
        }
    }
    return false;
}
__device__ __forceinline__ bool host_encap6(const EncapDev &H, uint32_t d0, uint32_t d1, uint32_t d2, uint32_t &tun_ip,
                                            uint32_t &ab) {
    if (H.encap_ifindex && d0 == H.node6[0] && d1 == H.node6[1] && d2 == H.node6[2]) {
        uint32_t tk[5] = {d0, d1, d2, 0u, 2u};          // daddr/96
        const int64_t ft = ht_find<20>(H.tunnel, tk, key_hash<20>(tk));
        ab += 20;
        if (ft >= 0) {
            tun_ip = __builtin_bswap32(gload<uint32_t>(ht_val(H.tunnel, ft)));
            ab += 20;
            return true;
        }
    }
    return false;
}

// from_netdev of bpf/bpf_netdev.c:395-460 -> handle_ipv4 (:326-393) / handle_ipv6 (:160-247),
// without FROM_HOST.  OPTS (k_nd_front; X is null without): the HANDLE_NS block, icmp6_handle
// (:180-186, lib/icmp6.h:380-401), and the ENCAP_IFINDEX branches (:225-243, :378-392), each
// behind its GF_NETDEV_F_* flag; k_pipe_front's instance is compiled without them.
enum { ND_RESPOND = 1004 };
template <bool OPTS>
__device__ int pipe_netdev(const NetdevDev &N, const NdxDev *X, FrontLane &L) {
    const Row &w = L.w;
    if (L.et == 0x0800) {
        if (L.len < 34) return D_INVALID;               // revalidate_data
        L.sec = (N.flags & GF_NETDEV_F_FIXED_SECCTX) ? N.fixed_secctx : 2u;   // derive_ipv4_sec_ctx: WORLD_ID
        const uint32_t da = w.r32(30);                  // post-LB daddr
        const uint8_t *ep = lxc_lookup4(N.lx, da, L.ab);
        if (!ep) {
            if constexpr (OPTS)
                if ((N.flags & GF_NETDEV_F_ENCAP) && host_encap4(X->enc, da, L.tun_ip, L.ab)) return HO_ENCAP;
            return TC_OK;
        }
        if (ep_is_host(ep)) return TC_OK;
        return local_delivery4(L, ep);
    }
    if (L.et == 0x86DD) {
        if (L.len < 54) return D_INVALID;
        if constexpr (OPTS) {
            // HANDLE_NS: nexthdr as ipv6_hdrlen left it (h.proto: a rejected chain keeps
            // ip6->nexthdr, never 58).  icmp6_load_type (icmp6.h:38-41) is load_byte at the fixed
            // ETH_HLEN + 40, also behind extension headers; a load past the frame ends the program
            // with 0 = TC_ACT_OK.
            if ((N.flags & GF_NETDEV_F_HANDLE_NS) && L.h.proto == 58) {
                if (L.len < 55) return TC_OK;
                const uint32_t type = w.b(54);
                L.ab += 1;
                if (type == 135) { L.call = GF_CALL_ICMP6_NS; return ND_RESPOND; }   // icmp6_handle_ns (:389-390)
                if (type == 128 && w.r32(38) == X->router6[0] && w.r32(42) == X->router6[1] &&
                    w.r32(46) == X->router6[2] && w.r32(50) == X->router6[3]) {   // :391-393
                    L.call = GF_CALL_ICMP6_ECHO_REPLY;
                    return ND_RESPOND;
                }
            }
        }
        L.sec = derive_sec_ctx6(w, N.flags, N.fixed_secctx, N.router6);
        const uint8_t *ep = lxc_lookup6(N.lx, w, L.ab);
        if (!ep) {
            if constexpr (OPTS)
                if ((N.flags & GF_NETDEV_F_ENCAP) && host_encap6(X->enc, w.r32(38), w.r32(42), w.r32(46), L.tun_ip, L.ab))
                    return HO_ENCAP;
            return TC_OK;
        }
        if (ep_is_host(ep)) return TC_OK;
        return local_delivery6(L, ep);
    }
    return TC_OK;                                       // unknown traffic to the stack
}

// ---- the front skeleton
// TRACE_FROM_*'s capture of the lane's row as it stands (128 B per packet); each entry calls it
// at its program's send_trace_notify.
__device__ __forceinline__ void front_capture(const FrontLane &L, uint8_t *tcap_in, uint32_t S, uint32_t vec_copy) {
    if (!tcap_in) return;
    uint8_t *d = tcap_in + (size_t)L.i * GF_TRACE_PAYLOAD_LEN;
    const uint32_t cb = S < GF_TRACE_PAYLOAD_LEN ? S : GF_TRACE_PAYLOAD_LEN;
    if (vec_copy) {
        for (uint32_t k = 0; k < cb; k += 16)
            *reinterpret_cast<uint4 *>(d + k) = *reinterpret_cast<const uint4 *>(L.w.p + k);
    } else {
        for (uint32_t k = 0; k < cb; k++) d[k] = L.w.p[k];
    }
}

// An entry program's return value in the record, once the entry has turned its own codes into
// actions: the port map's rewrite, the tail call, ICMPv6 time exceeded, a drop, or the action.
// SHOT_DROPS: TC_ACT_SHOT itself is a drop too (the netdev stage, whose LB stage returns it).
template <bool SHOT_DROPS>
__device__ __forceinline__ void front_result(FrontLane &L, int r, uint32_t stage) {
    gf_pipeline_out &o = L.o;
    if (L.mapped) { o.flags |= GF_PIPE_F_PORTMAP; o.dport = (uint16_t)L.ndport; }
    o.stage = (uint8_t)stage;
    if (r == ND_TAILCALL) { o.stage = GF_STAGE_POLICY; o.lxc_id = (uint16_t)L.lxc; L.tail = true; }
    else if (r == ND_ICMP6_TE) { o.action = TC_REDIRECT; o.flags |= GF_PIPE_F_ICMP6_TE; }
    else if (r < 0 || (SHOT_DROPS && r == TC_SHOT)) { o.action = TC_SHOT; o.reason = (uint8_t)(-r); }   // send_drop_notify_error
    else o.action = (uint8_t)r;
}

// One packet per lane.  The block's frames are staged in LDS (NT * snap_stride bytes of dynamic
// shared memory, <= 32 KiB) and copied back out only when the caller asked for the rewritten
// frames.  entry(L) runs the entry's programs on the lane's row; then the rewritten header is
// re-parsed and the packet's handle_policy record and flow-group key are written for ingress_run
// (k_ing_pack fused), and a packet that ended here is counted.
// CLS_FLAGS: the record's front flags (every GF_PIPE_F_* bit: the top three of the byte) ride
// along in cls bits 4-6 for k_ing_groups' write-only completion (IngCtx::pout_wo).
template <int NT, bool CLS_FLAGS, class Entry>
__device__ __forceinline__ void front_body(const gf_frames &fr, const uint8_t *tc_index, uint32_t vec_copy,
                                           const uint16_t *slot_of, gf_rec *rec, uint32_t *keys, uint8_t *s6out,
                                           uint8_t *d6out, gf_pipeline_out *out, uint8_t *snap_out,
                                           unsigned long long *stats, const gf_key_cfg &K, Entry entry) {
    extern __shared__ uint4 lds_rows[];
    uint8_t *rows = reinterpret_cast<uint8_t *>(lds_rows);
    __shared__ uint32_t sl[272];
    Stats st{sl};
    if (stats) st.init();
    const uint32_t S = fr.snap_stride;
    const uint32_t b0 = blockIdx.x * NT;
    const uint32_t nb = fr.n - b0 < NT ? fr.n - b0 : NT;
    const size_t bytes = (size_t)nb * S;
    {
        const uint8_t *src = fr.snap + (size_t)b0 * S;
        size_t k0 = 0;
        if (vec_copy) {
            const size_t nv = bytes / 16;
            for (size_t k = threadIdx.x; k < nv; k += NT) lds_rows[k] = reinterpret_cast<const uint4 *>(src)[k];
            k0 = nv * 16;
        }
        for (size_t k = k0 + threadIdx.x; k < bytes; k += NT) rows[k] = src[k];
    }
    __syncthreads();
    const uint32_t i = b0 + threadIdx.x;
    bool scnt = false;                                  // the lane's counter-block entry
    uint32_t sreason = 0, saction = 0, slen = 0, sab = 0;
    if (i < fr.n) {
        const uint32_t len = fr.len[i];
        const uint32_t cap = S < len ? S : len;
        FrontLane L{};
        L.i = i; L.len = len;
        L.w = Row{rows + (size_t)threadIdx.x * S, cap};
        parse_row(L.w.p, cap, len, L.h);
        L.et = L.h.et;
        L.ab = 24 + 34;                                 // output record, header bytes parsed
        entry(L);
        // handle_policy's input: the rewritten header, re-parsed
        gf_rec rr;
        uint32_t key;
        const uint32_t tci = (tc_index ? tc_index[i] : 0u) | L.tci_or;
        if (L.tail) {
            PktHdr h2;
            parse_row(L.w.p, cap, len, h2);
            key = pack_rec(i, h2.et, len, h2.sa, h2.da, h2.w0, h2.w3, h2.l4, h2.proto, L.sec, L.ifx,
                           slot_of[L.lxc & 0xffffu], tci, false, true, h2.s6, h2.d6, rr, K);
            if constexpr (CLS_FLAGS) {
                static_assert(((GF_PIPE_F_ICMP6_TE | GF_PIPE_F_LB | GF_PIPE_F_PORTMAP) & ~0xE0u) == 0,
                              "the pipeline's front flags must fit the top three bits of the flags byte");
                rr.cls |= (uint8_t)(((L.o.flags & 0xE0u) >> 5) << 4);
            }
            if (h2.et == 0x86DD) {                       // both addresses in one 32-B piece (a6_stride 32)
                reinterpret_cast<uint4 *>(s6out)[2 * (size_t)i] = make_uint4(h2.s6[0], h2.s6[1], h2.s6[2], h2.s6[3]);
                reinterpret_cast<uint4 *>(d6out)[2 * (size_t)i] = make_uint4(h2.d6[0], h2.d6[1], h2.d6[2], h2.d6[3]);
            }
        } else {
            key = pack_rec(i, L.et, len, 0, 0, 0, 0, 0, 0, L.keep_sec ? L.sec : 0u, 0, 0, tci, true, true, L.h.s6, L.h.d6,
                           rr, K);
        }
        rec[i] = rr;
        keys[i] = key;
        out[i] = L.o;
        sab = L.ab;                                     // a tail-called packet: handle_policy counts it
        if (!L.tail) { scnt = true; sreason = L.o.reason; saction = L.o.action; slen = len; }
    }
    if (stats) st.pkt_wave(scnt, sreason, saction, slen, sab);
    if (snap_out) {
        __syncthreads();
        uint8_t *dst = snap_out + (size_t)b0 * S;
        size_t k0 = 0;
        if (vec_copy) {
            const size_t nv = bytes / 16;
            for (size_t k = threadIdx.x; k < nv; k += NT) reinterpret_cast<uint4 *>(dst)[k] = lds_rows[k];
            k0 = nv * 16;
        }
        for (size_t k = k0 + threadIdx.x; k < bytes; k += NT) dst[k] = rows[k];
    }
    if (stats) st.flush(stats);
}

// bpf_xdp and bpf_lb from-netdev on the lane's row, ahead of the netdev program (k_pipe_front,
// k_nd_front).  n6: the LB's new IPv6 daddr, zero unless it translated.  false: the packet
// ended here and L.o says how.
__device__ __forceinline__ bool pipe_xdp_lb(const PipeDev &P, FrontLane &L, uint32_t fhash, uint32_t *n6) {
    const PktHdrA ha{L.h, fhash};
    gf_pipeline_out &o = L.o;
    if (P.has_xdp && xdp_verdict(P.x, ha, L.len, L.et, L.ab) == XDP_DROP_) {
        o.stage = GF_STAGE_XDP; o.action = XDP_DROP_;
        return false;
    }
    if (P.has_lb) {
        gf_lb_out lo{};
        uint32_t kd = 0;
        int ret = TC_OK;
        bool v6 = false;
        L.ab += 12;
        if (L.et == 0x86DD) {
            if (!(P.L.flags & GF_LB_F_NO_IPV6)) { v6 = true; L.ab += 28; ret = lb_v6(P.L, ha, L.len, lo, n6, L.ab, kd); }
        } else if (L.et == 0x0800) {
            if (!(P.L.flags & GF_LB_F_NO_IPV4)) ret = lb_v4(P.L, ha, L.len, lo, L.ab, kd);
        }
        if (ret < 0 || ret == TC_SHOT) {
            o.stage = GF_STAGE_LB; o.action = TC_SHOT; o.reason = (uint8_t)(-ret);
            n6[0] = n6[1] = n6[2] = n6[3] = 0;
            return false;
        }
        if (ret == TC_REDIRECT) {
            pipe_lb_rewrite(L.w, L.len, L.h, v6, lo, n6, kd, L.ab);
            o.slave = lo.slave; o.rev_nat = lo.rev_nat; o.dport = lo.new_dport;
            o.daddr4 = v6 ? 0u : lo.new_daddr4;
            o.flags |= GF_PIPE_F_LB;
            if (P.L.flags & GF_LB_F_REDIRECT) {
                o.stage = GF_STAGE_LB; o.action = TC_REDIRECT; o.ifindex_lo = (uint16_t)P.lb_redirect_ifindex;
                return false;
            }
        } else {
            n6[0] = n6[1] = n6[2] = n6[3] = 0;
        }
    }
    return true;
}
// ... and the packet's nd6 entry
__device__ __forceinline__ bool front_xdp_lb(const PipeDev &P, FrontLane &L, const uint32_t *flow_hash, uint8_t *nd6) {
    uint32_t n6[4] = {0, 0, 0, 0};
    const bool on = pipe_xdp_lb(P, L, flow_hash ? flow_hash[L.i] : 0u, n6);
    if (nd6) reinterpret_cast<uint4 *>(nd6)[L.i] = make_uint4(n6[0], n6[1], n6[2], n6[3]);
    return on;
}

template <int NT>
__global__ __launch_bounds__(NT, GF_FRONT_MINW) void k_pipe_front(gf_frames fr, const uint8_t *tc_index, const uint32_t *flow_hash,
                                                      PipeDev P, const uint16_t *slot_of, gf_rec *rec, uint32_t *keys,
                                                      uint8_t *s6out, uint8_t *d6out, gf_pipeline_out *out,
                                                      uint8_t *nd6, uint8_t *snap_out, unsigned long long *stats, gf_key_cfg K) {
    front_body<NT, true>(fr, tc_index, P.vec_copy, slot_of, rec, keys, s6out, d6out, out, snap_out, stats, K,
                         [&](FrontLane &L) {
        if (!front_xdp_lb(P, L, flow_hash, nd6)) return;
        front_capture(L, P.tcap_in, fr.snap_stride, P.vec_copy);   // from_netdev's send_trace_notify (bpf_netdev.c:436)
        front_result<true>(L, pipe_netdev<false>(P.nd, nullptr, L), GF_STAGE_NETDEV);
    });
}

// The pipeline whose netdev stage has GF_NETDEV_F_HANDLE_NS or GF_NETDEV_F_ENCAP; a pipeline
// that sets neither never gets here.  Not held to k_pipe_front's 64 VGPRs (<= 32 KiB of LDS
// rows: five blocks per CU).
template <int NT>
__global__ __launch_bounds__(NT) void k_nd_front(gf_frames fr, const uint8_t *tc_index, const uint32_t *flow_hash,
                                                 PipeDev P, NdxDev X, const uint16_t *slot_of, gf_rec *rec,
                                                 uint32_t *keys, uint8_t *s6out, uint8_t *d6out, gf_pipeline_out *out,
                                                 uint8_t *nd6, uint8_t *snap_out, unsigned long long *stats, gf_key_cfg K) {
    front_body<NT, true>(fr, tc_index, P.vec_copy, slot_of, rec, keys, s6out, d6out, out, snap_out, stats, K,
                         [&](FrontLane &L) {
        if (front_xdp_lb(P, L, flow_hash, nd6)) {
            front_capture(L, P.tcap_in, fr.snap_stride, P.vec_copy);
            const int r = pipe_netdev<true>(P.nd, &X, L);
            const bool respond = r == ND_RESPOND, encap = r == HO_ENCAP;
            L.o.flags |= respond ? GF_PIPE_F_RESPONDER : encap ? GF_PIPE_F_ENCAP : 0u;
            L.o.pad0 = (uint8_t)L.call;                 // 0 unless a responder call: action OK, reason 0 (as eg_front6)
            if (encap) L.o.ifindex_lo = (uint16_t)X.enc.encap_ifindex;
            L.keep_sec = encap;
            front_result<true>(L, respond ? TC_OK : encap ? TC_REDIRECT : r, GF_STAGE_NETDEV);
        }
        if (X.tunnel_ip) X.tunnel_ip[L.i] = L.tun_ip;
    });
}

// ================================================================ bpf_lb over frames
// from_netdev of bpf/bpf_lb.c:169-212 on a node in lb mode (bpf/init.sh:341-342), where the
// program is the whole datapath: dispatch on the ethertype, handle_ipv4 / handle_ipv6
// (lb_v4 / lb_v6, shared with k_lb and the pipeline's LB stage), lb4_xlate / lb6_xlate
// (pipe_lb_rewrite), LB_DSTMAC (:200-205), the record of gf_lb_classify.  Not on front_body:
// that skeleton exists to hand a gf_rec, a flow-group key and a pipeline record per frame to
// ingress_run (60 B a frame), none of which this program has a reader for.  It keeps the
// skeleton's tile: the block's rows staged in LDS by coalesced 16-B loads, one frame per lane
// over its row there (DESIGN.md §3 has the reasoning against per-lane global loads).
// What leaves the tile depends on dst:
//   null            nothing but the record;
//   the input rows  (in place) a translated frame's lane stores the fields the program wrote,
//                   from its LDS row, and nothing else: an untouched frame is not written;
//   another buffer  the whole tile, patches included, by coalesced 16-B stores.
struct LbFrDev {
    uint32_t has_mac, mac_lo, mac_hi;  // LB_DSTMAC as eth_store_daddr writes it: bytes 0-3, 4-5
    uint32_t vec_copy;
};
// bytes [off, off + n) of the lane's row to the same place of its frame in global memory
// (past the row's cap: dropped, as Row::w8 drops them)
__device__ __forceinline__ void lbf_put(const Row &w, uint8_t *g, uint32_t off, uint32_t n) {
    for (uint32_t k = off; k < off + n; k++)
        if (k < w.cap) g[k] = w.p[k];
}
template <int NT>
__global__ __launch_bounds__(NT) void k_lb_frames(gf_frames fr, const uint32_t *flow_hash, LbDev L, LbFrDev F,
                                                  gf_lb_out *out, uint8_t *nd6, uint8_t *dst,
                                                  unsigned long long *stats) {
    extern __shared__ uint4 lbf_rows[];
    uint8_t *rows = reinterpret_cast<uint8_t *>(lbf_rows);
    __shared__ uint32_t sl[272];
    Stats st{sl};
    if (stats) st.init();
    const uint32_t S = fr.snap_stride;
    const uint32_t b0 = blockIdx.x * NT;
    const uint32_t nb = fr.n - b0 < NT ? fr.n - b0 : NT;
    const size_t bytes = (size_t)nb * S;
    {
        const uint8_t *src = fr.snap + (size_t)b0 * S;
        size_t k0 = 0;
        if (F.vec_copy) {
            const size_t nv = bytes / 16;
            for (size_t k = threadIdx.x; k < nv; k += NT) lbf_rows[k] = reinterpret_cast<const uint4 *>(src)[k];
            k0 = nv * 16;
        }
        for (size_t k = k0 + threadIdx.x; k < bytes; k += NT) rows[k] = src[k];
    }
    __syncthreads();
    const uint32_t i = b0 + threadIdx.x;
    const bool act = i < fr.n;
    const bool inplace = dst == fr.snap;
    gf_lb_out o{};
    uint32_t len = 0, ab = 0;
    if (act) {
        len = fr.len[i];
        Row w{rows + (size_t)threadIdx.x * S, S < len ? S : len};
        PktHdr h;
        parse_row(w.p, w.cap, len, h);
        ab = 12 + 34;                                   // output record, header bytes parsed
        const PktHdrA ha{h, flow_hash ? flow_hash[i] : 0u};
        uint32_t n6[4] = {0, 0, 0, 0};
        int ret = TC_OK;
        bool v6 = false;
        uint32_t kd = 0;
        if (h.et == 0x86DD) { if (!(L.flags & GF_LB_F_NO_IPV6)) { v6 = true; ab += 28; ret = lb_v6(L, ha, len, o, n6, ab, kd); } }
        else if (h.et == 0x0800) { if (!(L.flags & GF_LB_F_NO_IPV4)) ret = lb_v4(L, ha, len, o, ab, kd); }
        if (ret < 0 || ret == TC_SHOT) {                // send_drop_notify_error(skb, ret, TC_ACT_SHOT)
            o = gf_lb_out{};
            o.action = TC_SHOT; o.reason = (uint8_t)(-ret);
            n6[0] = n6[1] = n6[2] = n6[3] = 0;
        } else {
            o.action = ((L.flags & GF_LB_F_REDIRECT) && ret == TC_REDIRECT) ? TC_REDIRECT : TC_OK;
        }
        if (ret == TC_REDIRECT && dst) {
            pipe_lb_rewrite(w, len, h, v6, o, n6, kd, ab);
            const bool mac = o.action == TC_REDIRECT && F.has_mac;
            if (mac) { w.w32(0, F.mac_lo); w.w16(4, F.mac_hi); ab += 6; }   // eth_store_daddr(skb, mac.addr, 0)
            if (inplace) {
                uint8_t *g = dst + (size_t)i * S;
                const uint32_t co = csum_l4_offset(h.proto);
                if (mac) lbf_put(w, g, 0, 6);
                if (!v6) { lbf_put(w, g, 24, 2); lbf_put(w, g, 30, 4); }
                else lbf_put(w, g, 38, 16);
                if (co || v6) lbf_put(w, g, (uint32_t)h.l4 + co, 2);
                if (o.new_dport) lbf_put(w, g, (uint32_t)h.l4 + 2, 2);
            }
        }
        out[i] = o;
        if (nd6) reinterpret_cast<uint4 *>(nd6)[i] = make_uint4(n6[0], n6[1], n6[2], n6[3]);
    }
    if (stats) st.pkt_wave(act, o.reason, o.action, len, ab);
    if (dst && !inplace) {
        __syncthreads();
        uint8_t *d = dst + (size_t)b0 * S;
        size_t k0 = 0;
        if (F.vec_copy) {
            const size_t nv = bytes / 16;
            for (size_t k = threadIdx.x; k < nv; k += NT) reinterpret_cast<uint4 *>(d)[k] = lbf_rows[k];
            k0 = nv * 16;
        }
        for (size_t k = k0 + threadIdx.x; k < bytes; k += NT) d[k] = rows[k];
    }
    if (stats) st.flush(stats);
}

// ================================================================ from-overlay
// from_overlay of bpf/bpf_overlay.c:167-200 -> handle_ipv4 (:106-153) /
// handle_ipv6 (:38-102), VXLAN (ENCAP_GENEVE undefined), ENABLE_IPV4: the
// program on the tunnel device.  Each frame is the inner frame; its
// bpf_tunnel_key.tunnel_id (the sender's identity) comes as a column.  Not
// modelled: skb_get_tunnel_key failing (DROP_NO_TUNNEL_KEY, it cannot fail for a
// frame the tunnel device received).
// ENCAP_GENEVE (GF_OVERLAY_F_GENEVE) is the GENEVE instance of the front: handle_ipv6's
// block :54-67, skb_get_tunnel_opt + parse_geneve_options (lib/geneve.h:46-60), between
// the length check and the endpoint lookup.  handle_ipv4 has no such block.  The lane's
// options come as two columns (OvlOpt); only the first word of the 64-byte buffer is ever
// looked at, so that is all the kernel loads.
template <bool GENEVE> struct OvlOpt {};               // VXLAN: no kernel argument bytes beyond the empty struct
template <> struct OvlOpt<true> {
    const uint8_t *opt;            // n * stride, 4-byte aligned rows (gf_tunnel_opts)
    const uint8_t *len;            // options_len per packet
    uint32_t stride;
};
struct OvlDev {
    LxcDev lx;
    uint32_t host_ifindex;         // HOST_IFINDEX, 0 = undefined (to_host is TC_ACT_OK)
    uint32_t host_mac[2], node_mac[2];   // HOST_IFINDEX_MAC, NODE_MAC (LE words)
    uint32_t vec_copy;
    uint8_t *tcap_in;              // TRACE_FROM_OVERLAY captures (128 B per packet; null: no trace)
};
enum { OV_TO_HOST = 1002 };

// to_host (:134-149, :83-98), after ipv4_l3 / ipv6_l3 decremented the TTL
__device__ __forceinline__ int ovl_to_host(const OvlDev &O, FrontLane &L) {
    L.w.w32(6, O.node_mac[0]); L.w.w16(10, O.node_mac[1]);   // eth_store_saddr(NODE_MAC)
    L.w.w32(0, O.host_mac[0]); L.w.w16(4, O.host_mac[1]);    // eth_store_daddr(HOST_IFINDEX_MAC)
    L.ab += 12;
    return OV_TO_HOST;
}

// gw / gl (GENEVE): the first word of the lane's option buffer as skb_get_tunnel_opt leaves it
// (bytes past options_len zero) and options_len.
template <bool GENEVE>
__device__ int ovl_program(const OvlDev &O, FrontLane &L, uint32_t gw, uint32_t gl) {
    if (L.et == 0x0800) {
        if (L.len < 34) return D_INVALID;               // revalidate_data (:114-115)
        const uint8_t *ep = lxc_lookup4(O.lx, L.w.r32(30), L.ab);   // lookup_ip4_endpoint (:123)
        if (!ep) return D_NON_LOCAL;                    // :130-131
        if (!ep_is_host(ep)) return local_delivery4(L, ep);   // :129
        if (!O.host_ifindex) return TC_OK;              // HOST_IFINDEX undefined (:150-151)
        if (const int e = dec_ttl4(L)) return e;        // ipv4_l3 (l3.h:54-69)
        return ovl_to_host(O, L);
    }
    if (L.et == 0x86DD) {
        if (L.len < 54) return D_INVALID;               // :46-47
        if constexpr (GENEVE) {
            // bpf_skb_get_tunnel_opt (net/core/filter.c): -ENOENT without options, -ENOMEM past the buffer (:60-61)
            if (gl == 0 || gl > 64) return D_NO_TUNNEL_OPT;
            L.ab += 1 + 4;
            // parse_geneve_options (:63-65): class 0xffff, type 1, (length & 0x1f) << 2 == 4; r1-r3 ignored
            if ((gw & 0x1fffffffu) != 0x0101ffffu) return D_INVALID_GENEVE;
        }
        const uint8_t *ep = lxc_lookup6(O.lx, L.w, L.ab);   // lookup_ip6_endpoint (:70)
        if (!ep) return D_NON_LOCAL;                    // :79-80
        if (!ep_is_host(ep)) return local_delivery6(L, ep);   // :78
        if (!O.host_ifindex) return TC_OK;              // :99-100
        if (const int e = dec_hoplimit6(L)) return e;   // ipv6_l3 (l3.h:31-52)
        return ovl_to_host(O, L);
    }
    return TC_OK;                                       // unknown traffic to the stack (:191-193)
}

// The tunnel device's entry; the source identity is the frame's tunnel id.  Not held to
// k_pipe_front's 64 VGPRs (<= 32 KiB of LDS rows: five blocks per CU).
// GENEVE: the lane's option word and options_len are two coalesced column loads issued
// before the frame-row copy (registers, no LDS); the VXLAN instances compile without them.
template <int NT, bool GENEVE>
__global__ __launch_bounds__(NT) void k_ovl_front(gf_frames fr, const uint32_t *tunnel_id, const uint8_t *tc_index,
                                                  OvlDev O, const uint16_t *slot_of, gf_rec *rec, uint32_t *keys,
                                                  uint8_t *s6out, uint8_t *d6out, gf_pipeline_out *out,
                                                  uint8_t *snap_out, unsigned long long *stats, gf_key_cfg K,
                                                  OvlOpt<GENEVE> G) {
    uint32_t gw = 0, gl = 0;
    if constexpr (GENEVE) {
        const uint32_t i = blockIdx.x * NT + threadIdx.x;
        if (i < fr.n) {
            gl = G.len[i];
            gw = *reinterpret_cast<const uint32_t *>(G.opt + (size_t)i * G.stride);
            // the zero-initialised buffer past options_len (gl > 64 is refused before the word is looked at)
            if (gl < 4) gw &= (1u << (8 * gl)) - 1u;
        }
    }
    front_body<NT, true>(fr, tc_index, O.vec_copy, slot_of, rec, keys, s6out, d6out, out, snap_out, stats, K,
                         [&](FrontLane &L) {
        L.ab += 4;                                      // the tunnel id
        front_capture(L, O.tcap_in, fr.snap_stride, O.vec_copy);   // from_overlay's send_trace_notify (:174): the frame as received
        int r = ovl_program<GENEVE>(O, L, gw, gl);
        if (r == OV_TO_HOST) { r = TC_REDIRECT; L.o.ifindex_lo = (uint16_t)O.host_ifindex; }
        front_result<false>(L, r, GF_STAGE_OVERLAY);
        if (L.tail) L.sec = tunnel_id[L.i];
    });
}

// encap_and_redirect's bpf_tunnel_key.tunnel_id and GENEVE_OPTS (lib/encap.h:43, 53, 72-81) for
// the records of a from-container call (gf_lxc_egress_tunnel_meta): one packet per lane, the
// sender's program through the cilium_policy slot table as k_ing_pack reads it.
__global__ __launch_bounds__(BLOCK) void k_tun_meta(const uint16_t *lxc_id, const gf_egress_out *recs, uint32_t n,
                                                    const uint16_t *slot_of, const gf_lxc_dev *cfgs,
                                                    uint32_t *tunnel_id, uint32_t *opt, uint8_t *opt_len) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    uint32_t tid = 0, w0 = 0, w1 = 0, ol = 0;
    if (recs[i].eg_flags & GF_EG_F_ENCAP) {
        const uint32_t slot = slot_of[lxc_id[i]];
        if (slot) {                                     // (an encap record always has a program)
            tid = gload<uint32_t>(&cfgs[slot - 1].seclabel);
            w0 = 0x0101ffffu;                           // ff ff 01 01: class, type, len >> 2
            w1 = __builtin_bswap32(tid);                // the identity, big-endian
            ol = 8;
        }
    }
    tunnel_id[i] = tid;
    opt[2 * (size_t)i] = w0;
    opt[2 * (size_t)i + 1] = w1;
    opt_len[i] = (uint8_t)ol;
}

// ================================================================ from-host
// from_netdev of bpf/bpf_netdev.c:414-468 -> handle_ipv4 (:328-396) / handle_ipv6
// (:163-246) compiled with FROM_HOST and ENABLE_IPV4, without HANDLE_NS; ENCAP_IFINDEX
// is defined iff encap_ifindex != 0: the program on cilium_host.  skb->mark comes as
// a column; its reset to 0 (:143) has no output.  The reverse lookups read
// cilium_proxy{4,6} as they stand when the kernel runs, which is before
// handle_policy of the same call inserts anything (the inserts are applied after
// k_ing_groups, see px_log_apply).
struct HostDev {
    LxcDev lx;
    EncapDev enc;
    gf_htab_desc px4, px6;
    uint32_t flags, fixed_secctx;  // GF_NETDEV_F_*, FIXED_SRC_SECCTX
    uint32_t router6[2];           // first 8 bytes of the netdev's ROUTER_IP (derive_sec_ctx)
    uint32_t net_mac[2];           // CILIUM_NET_MAC (LE words)
    uint32_t vec_copy;
    uint8_t *tcap_in;              // TRACE_FROM_HOST / FROM_PROXY captures (128 B per packet; null: no trace)
};
enum { MARK_MAGIC_PROXY_MASK = 0xFFF, MARK_MAGIC_PROXY_INGRESS = 0xFEA, MARK_MAGIC_PROXY_EGRESS = 0xFEB };

// handle_identity_from_proxy (:128-145): the identity the proxy put into the mark
// (0: none), skip = TC_INDEX_F_SKIP_PROXY for the ingress proxy's packets.
__device__ __forceinline__ uint32_t host_mark_identity(uint32_t mark, uint32_t &skip) {
    const uint32_t magic = mark & MARK_MAGIC_PROXY_MASK;
    skip = magic == MARK_MAGIC_PROXY_INGRESS ? 1u : 0u;
    return (magic == MARK_MAGIC_PROXY_INGRESS || magic == MARK_MAGIC_PROXY_EGRESS) ? mark >> 16 : 0u;
}

// reverse_proxy (:264-325) / reverse_proxy6 (:67-124); nh is the IP header's own
// next-header byte (an IPv6 frame with an extension header is ignored).  rev: the
// translation was applied.
__device__ int host_reverse_proxy(const HostDev &H, Row &w, uint32_t len, bool v6, int l4_off, uint32_t nh,
                                  uint32_t &rev, uint32_t &ab) {
    if (nh != 6 && nh != 17) return 0;
    if (!skb_ok(l4_off, 4, len)) return D_CT_INVALID_HDR;
    const uint32_t ports = w.r32((uint32_t)l4_off);     // key.dport = the packet's sport, key.sport = its dport
    const uint32_t co = csum_l4_offset(nh), fl = nh == 17 ? GF_F_MANGLED_0 : 0u;
    ab += 4;
    if (!v6) {
        uint32_t kw[3] = {w.r32(30), ports, nh};        // .saddr = ip4->daddr
        const int64_t f = ht_find<10>(H.px4, kw, key_hash<10>(kw));
        ab += 10;
        if (f < 0) return 0;
        const uint8_t *v = ht_val(H.px4, f);
        const uint32_t new_saddr = gload<uint32_t>(v), new_sport = gload<uint16_t>(v + 4);
        const uint32_t old_saddr = w.r32(26), old_sport = ports & 0xffffu;
        ab += 16;
        if (l4_csum(w, len, l4_off + (int)co, old_sport, new_sport, 2u | fl) < 0) return D_WRITE_ERROR;   // l4_modify_port
        w.w16((uint32_t)l4_off, new_sport);
        w.w32(26, new_saddr);
        l3_csum(w, len, 24, old_saddr, new_saddr, 4);
        l4_csum(w, len, l4_off + (int)co, old_saddr, new_saddr, 4u | GF_F_PSEUDO_HDR | fl);
        ab += 2 + 4 + 2 + 2;
    } else {
        uint32_t kw[6] = {w.r32(38), w.r32(42), w.r32(46), w.r32(50), ports, nh};   // .saddr = ip6->daddr
        const int64_t f = ht_find<22>(H.px6, kw, key_hash<22>(kw));
        ab += 22;
        if (f < 0) return 0;
        const uint8_t *v = ht_val(H.px6, f);
        const uint32_t new_sport = gload<uint16_t>(v + 16), old_sport = ports & 0xffffu;
        ab += 28;
        if (l4_csum(w, len, l4_off + (int)co, old_sport, new_sport, 2u | fl) < 0) return D_WRITE_ERROR;   // l4_modify_port
        w.w16((uint32_t)l4_off, new_sport);
        uint32_t sum = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) {                   // ipv6_store_saddr + csum_diff(old, 16, new, 16, 0)
            const uint32_t o = w.r32(22 + 4 * k), nw = gload<uint32_t>(v + 4 * k);
            w.w32(22 + 4 * k, nw);
            sum = ck_add(ck_add(sum, ~o), nw);
        }
        l4_csum(w, len, l4_off + (int)co, 0, sum, GF_F_PSEUDO_HDR | fl);
        ab += 2 + 16 + 2;
    }
    rev = 1;
    return 0;
}

// pid: the proxy's identity from the mark (0: none)
__device__ int host_program(const HostDev &H, FrontLane &L, uint32_t pid) {
    Row &w = L.w;
    if (L.et == 0x0800) {
        if (L.len < 34) return D_INVALID;               // revalidate_data (:337-338)
        L.sec = (H.flags & GF_NETDEV_F_FIXED_SECCTX) ? H.fixed_secctx : 2u;   // derive_ipv4_sec_ctx: WORLD_ID
        if (pid) L.sec = pid;                           // :348-349
        const int rr = host_reverse_proxy(H, w, L.len, false, L.h.l4, w.b(23), L.rev, L.ab);   // :351
        if (rr < 0) return rr;
        w.w32(0, H.net_mac[0]); w.w16(4, H.net_mac[1]); // rewrite_dmac_to_host (:358)
        L.ab += 6;
        const uint32_t da = w.r32(30);
        const uint8_t *ep = lxc_lookup4(H.lx, da, L.ab);   // lookup_ip4_endpoint (:369)
        if (ep) {
            if (ep_is_host(ep)) return TC_OK;           // :372-373
            return local_delivery4(L, ep);              // :375
        }
        if (host_encap4(H.enc, da, L.tun_ip, L.ab)) return HO_ENCAP;   // ENCAP_IFINDEX (:378-393)
        return TC_OK;                                   // :395
    }
    if (L.et == 0x86DD) {
        if (L.len < 54) return D_INVALID;               // :174-175
        L.sec = derive_sec_ctx6(w, H.flags, H.fixed_secctx, H.router6);
        if (pid) L.sec = pid;                           // :195-196
        const int rr = host_reverse_proxy(H, w, L.len, true, L.h.l4, w.b(20), L.rev, L.ab);   // :198, ip6->nexthdr
        if (rr < 0) return rr;
        w.w32(0, H.net_mac[0]); w.w16(4, H.net_mac[1]); // rewrite_dmac_to_host (:205)
        L.ab += 6;
        const uint8_t *ep = lxc_lookup6(H.lx, w, L.ab); // lookup_ip6_endpoint (:216)
        if (ep) {
            if (ep_is_host(ep)) return TC_OK;           // :219-220
            return local_delivery6(L, ep);              // :222
        }
        if (host_encap6(H.enc, w.r32(38), w.r32(42), w.r32(46), L.tun_ip, L.ab)) return HO_ENCAP;   // :225-243
        return TC_OK;                                   // :245
    }
    return TC_OK;                                       // unknown traffic to the stack (:462-464)
}

// cilium_host's entry.  The record keeps GF_PIPE_F_REV_PROXY itself (bit 4 is not among the
// bits gf_rec.cls carries), so the host side has handle_policy complete the records by
// read-modify-write (PolicyPass::keep_flags) and not write-only.
template <int NT>
__global__ __launch_bounds__(NT) void k_host_front(gf_frames fr, const uint32_t *mark, const uint8_t *tc_index,
                                                   HostDev H, const uint16_t *slot_of, gf_rec *rec, uint32_t *keys,
                                                   uint8_t *s6out, uint8_t *d6out, gf_pipeline_out *out,
                                                   uint8_t *snap_out, unsigned long long *stats, gf_key_cfg K) {
    front_body<NT, false>(fr, tc_index, H.vec_copy, slot_of, rec, keys, s6out, d6out, out, snap_out, stats, K,
                          [&](FrontLane &L) {
        L.ab += 4;                                      // the mark
        uint32_t skip = 0;
        const uint32_t pid = host_mark_identity(mark ? mark[L.i] : 0u, skip);   // :425
        front_capture(L, H.tcap_in, fr.snap_stride, H.vec_copy);   // from_netdev's send_trace_notify (:433): the frame as received
        int r = host_program(H, L, pid);
        if (L.rev) { L.o.flags |= GF_PIPE_F_REV_PROXY; skip = 1; }   // :121, :320
        if (r == HO_ENCAP) {
            r = TC_REDIRECT; L.o.ifindex_lo = (uint16_t)H.enc.encap_ifindex; L.o.daddr4 = L.tun_ip;
            L.keep_sec = true;
        }
        front_result<false>(L, r, GF_STAGE_HOST);
        L.tci_or = skip;
    });
}

// ---- ingest re-partition (real traffic on N GPUs): the owner rank of each
// frame is the rank of its flow group, the unordered address pair that the
// CT of handle_policy sees, i.e. after bpf_lb's translation (stateless, so it
// can run before the exchange).  Same rule as the synthetic stream's
// (cilium_amd/stream.py pair_rank): fmix64 of (max << 32 | min) of the
// host-order addresses, mod the rank count.  Frames that cannot reach
// conntrack stay on their rank.
__device__ __forceinline__ uint32_t pair_rank4(uint32_t sa_raw, uint32_t da_raw, uint32_t world) {
    const uint64_t a = __builtin_bswap32(sa_raw), b = __builtin_bswap32(da_raw);
    uint64_t x = ((a < b ? b : a) << 32) | (a < b ? a : b);
    x ^= x >> 33; x *= 0xff51afd7ed558ccdull; x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ull; x ^= x >> 33;
    return (uint32_t)(x & 0xffffffffull) % world;
}
// lb_v6's translated address (d6 unchanged unless it translates); kept out of
// line: inlined into k_partition, the hipcc of this image merged the target's
// third word with the lookup key's (observed on gfx950, the parity test pins it)
__device__ __attribute__((noinline)) void lb_v6_daddr(const LbDev &L, const PktHdr &h, uint32_t fh, uint32_t len,
                                                      uint32_t *d6) {
    const PktHdrA ha{h, fh};
    gf_lb_out lo{};
    uint32_t n6[4], ab = 0, kd = 0;
    if (lb_v6(L, ha, len, lo, n6, ab, kd) == TC_REDIRECT)
        for (int k = 0; k < 4; k++) d6[k] = n6[k];
}
__global__ __launch_bounds__(BLOCK) void k_partition(gf_frames fr, const uint32_t *flow_hash, PipeDev P, uint32_t self,
                                                     uint32_t world, uint32_t *owner, uint32_t *counts) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= fr.n) return;
    const uint32_t len = fr.len[i], S = fr.snap_stride;
    const uint32_t cap = S < len ? S : len;
    PktHdr h;
    parse_row(fr.snap + (size_t)i * S, cap, len, h);
    const PktHdrA ha{h, flow_hash ? flow_hash[i] : 0u};
    uint32_t r = self, ab = 0, kd = 0;
    if (h.et == 0x0800 && len >= 34) {
        uint32_t da = h.da;
        if (P.has_lb && !(P.L.flags & GF_LB_F_NO_IPV4)) {
            gf_lb_out lo{};
            if (lb_v4(P.L, ha, len, lo, ab, kd) == TC_REDIRECT) da = lo.new_daddr4;
        }
        r = pair_rank4(h.sa, da, world);
    } else if (h.et == 0x86DD && len >= 54) {
        // lb_v6 leaves d6 alone unless it translates (then it writes all four words)
        uint32_t d6[4] = {h.d6[0], h.d6[1], h.d6[2], h.d6[3]};
        if (P.has_lb && !(P.L.flags & GF_LB_F_NO_IPV6)) lb_v6_daddr(P.L, h, ha.fh, len, d6);
        r = gf_pair_hash6(h.s6, d6) % world;
    }
    owner[i] = r;
    atomicAdd(&counts[r], 1u);
}

// ================================================================ CT garbage collection / LRU eviction
// ctmap.GC / Flush (pkg/maps/ctmap/ctmap.go:277-368, GCFilterByTime): delete every
// entry with lifetime < filter_time.  The LRU stand-in (below) deletes by the same
// sweep with two cutoffs: closing entries (rx_closing or tx_closing set) with
// lifetime < cut_c, the others with lifetime < cut_o.  On the device the sweep
// also compacts each probe cluster (a maximal run of non-EMPTY slots) in place,
// so deleted entries and the tombstones of ct_delete leave EMPTY slots behind:
// k_gc_starts marks the cluster starts (a non-EMPTY slot after an EMPTY one) on
// the unmodified table, then k_gc_clusters walks each cluster with one lane,
// dropping deleted entries and tombstones and moving every live entry to the
// first EMPTY slot at or after its home — the invariant lookups rely on (no
// EMPTY slot between a key's home and the key) holds after the move.
// Cutoffs live in device memory so an eviction decided on the device (no host
// round trip) runs the same two kernels; active == 0 makes them no-ops.
struct GcCut {
    unsigned long long c, o;      // closing / other entries: deleted iff their age key < cut
    uint32_t active;
    uint32_t lru;                 // age key: 0 = lifetime (ctmap.GC), 1 = last use (the LRU stand-in)
};
// One bit word of the cluster-start bits (32 slots from slot 32 * w) of table d.
__device__ __forceinline__ void gc_starts_word(const gf_htab_desc &d, uint32_t *bits, uint64_t w) {
    uint32_t m = 0;
    uint64_t i0 = w * 32;
    uint32_t prev = d.slots[((i0 - 1) & d.mask) * d.slot_size + d.ksz];
    for (int k = 0; k < 32; k++) {
        uint64_t i = i0 + k;
        if (i > d.mask) break;
        uint32_t st = d.slots[i * d.slot_size + d.ksz];
        if (st != GF_SLOT_EMPTY && prev == GF_SLOT_EMPTY) m |= 1u << k;
        prev = st;
    }
    bits[w] = m;
}
__global__ __launch_bounds__(BLOCK) void k_gc_starts(gf_htab_desc d, uint32_t *bits, const GcCut *cut) {
    if (!cut->active) return;
    const uint64_t nw = (d.mask + 1 + 31) / 32;
    for (uint64_t w = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; w < nw; w += (uint64_t)gridDim.x * blockDim.x)
        gc_starts_word(d, bits, w);
}

__device__ __forceinline__ void gc_move(const gf_htab_desc &d, uint64_t from, uint64_t to, uint32_t vstride) {
    uint8_t *a = d.slots + from * d.slot_size, *b = d.slots + to * d.slot_size;
    for (uint32_t k = 0; k < d.slot_size; k += 16) *reinterpret_cast<uint4 *>(b + k) = *reinterpret_cast<const uint4 *>(a + k);
    if (vstride) {
        uint8_t *va = d.vals + from * vstride, *vb = d.vals + to * vstride;
        if (vstride % 16 == 0)
            for (uint32_t k = 0; k < vstride; k += 16) *reinterpret_cast<uint4 *>(vb + k) = *reinterpret_cast<const uint4 *>(va + k);
        else
            for (uint32_t k = 0; k < vstride; k += 4) *reinterpret_cast<uint32_t *>(vb + k) = *reinterpret_cast<const uint32_t *>(va + k);
    }
    a[d.ksz] = GF_SLOT_EMPTY;
}

// lt_off: byte offset of ct_entry.lifetime within the value bytes ht_val points at
// (0 in the CT codec's hot block, 32 in the reference layout); the flags word
// follows it in both.  res[0] += deleted entries, res[1] += tombstones cleared.
// The time of an entry's last update: every writer of ct_entry.lifetime sets it to
// now + the timeout its flags select (conntrack.h:47-62, 127, 527): CT_CLOSE_TIMEOUT
// once both directions close, CT_DEFAULT_LIFETIME after a non-SYN packet, else
// CT_SYN_TIMEOUT.  lifetime - that timeout is exact to the second.
__device__ __forceinline__ long long ct_last_use(uint32_t lt, uint32_t fl) {
    const uint32_t to = ((fl & F_RX_CLOSING) && (fl & F_TX_CLOSING)) ? 10u : ((fl & F_SEEN_NON_SYN) ? 43200u : 300u);
    return (long long)lt - (long long)to;
}
__device__ __forceinline__ bool gc_kill(uint32_t lt, uint32_t fl, const GcCut &c) {
    const long long k = c.lru ? ct_last_use(lt, fl) : (long long)lt;
    const unsigned long long cut = (fl & (F_RX_CLOSING | F_TX_CLOSING)) ? c.c : c.o;
    return k < 0 || (unsigned long long)k < cut;
}
// The clusters that start in bit word w of table d: every walk stays inside d (it
// wraps at d.mask and ends at an EMPTY slot of d).
__device__ __forceinline__ void gc_clusters_word(const gf_htab_desc &d, uint32_t mode, uint32_t lt_off, const GcCut &cut,
                                                 uint32_t vstride, const uint32_t *bits, uint64_t w, uint32_t &dead,
                                                 uint32_t &tombs) {
    uint32_t m = bits[w];
    while (m) {
        const int k = __builtin_ctz(m);
        m &= m - 1;
        uint64_t j = w * 32 + k;
        // hole: a slot of this cluster before j was emptied by this walk.  Until
        // then every slot from the cluster start to j is occupied, so the entry
        // at j (whose home lies in that range) cannot move: no rehash needed.
        bool hole = false;
        for (;;) {
            uint8_t *sl = d.slots + j * d.slot_size;
            const uint32_t st = sl[d.ksz];
            if (st == GF_SLOT_EMPTY) break;
            if (st == GF_SLOT_TOMB || st == GF_SLOT_FREE) {
                sl[d.ksz] = GF_SLOT_EMPTY;
                tombs++;
                hole = true;
            } else {
                const uint8_t *v = ht_val(d, j) + lt_off;
                const uint32_t lt = *reinterpret_cast<const uint32_t *>(v);
                const uint32_t fl = *reinterpret_cast<const uint16_t *>(v + 4);
                if (gc_kill(lt, fl, cut)) {
                    sl[d.ksz] = GF_SLOT_EMPTY;
                    dead++;
                    hole = true;
                } else if (hole) {
                    uint32_t kw[10];
                    for (uint32_t q = 0; q < 10; q++) kw[q] = 0;
                    for (uint32_t q = 0; q < d.ksz; q += 4) {       // slots are 4-B aligned
                        const uint32_t x = *reinterpret_cast<const uint32_t *>(sl + q);
                        kw[q >> 2] = d.ksz - q >= 4 ? x : (x & ((1u << (8 * (d.ksz - q))) - 1u));
                    }
                    const uint64_t home = gf_home_slot(gf_key_hash(kw, d.ksz, mode), d.mask, d.slot_size);
                    for (uint64_t p = home; p != j; p = (p + 1) & d.mask) {
                        if (d.slots[p * d.slot_size + d.ksz] == GF_SLOT_EMPTY) { gc_move(d, j, p, vstride); break; }
                    }
                }
            }
            j = (j + 1) & d.mask;
        }
    }
}
__global__ __launch_bounds__(BLOCK) void k_gc_clusters(gf_htab_desc d, uint32_t mode, uint32_t lt_off, const GcCut *cutp,
                                                       const uint32_t *bits, unsigned long long *res) {
    if (!cutp->active) return;
    const GcCut cut = *cutp;
    const uint64_t nw = (d.mask + 1 + 31) / 32;
    const uint32_t vstride = d.vals ? (d.sstride ? d.sstride : d.vsz) : 0u;
    uint32_t dead = 0, tombs = 0;
    for (uint64_t w = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; w < nw; w += (uint64_t)gridDim.x * blockDim.x)
        gc_clusters_word(d, mode, lt_off, cut, vstride, bits, w, dead, tombs);
    if (dead) atomicAdd(&res[0], (unsigned long long)dead);
    if (tombs) atomicAdd(&res[1], (unsigned long long)tombs);
}

// The same sweep over several CT maps at once (gf_ct_gc_maps: a GC round over the
// per-endpoint maps of the ConntrackLocal option).  Up to GF_GC_MULTI maps travel in the
// kernel arguments.  The work of a launch is the maps' bit words laid end to end in
// tiles of BLOCK words, each map's words rounded up to whole tiles, so that a tile
// lies in one map: t0[k] is map k's first tile and a block finds its tile's map by a
// scan of t0[] in the arguments (block-uniform, no load from device memory), then
// runs the one-map bodies on that map's descriptor and its own word index.  The
// cutoff is a launch argument; each map's {deleted, tombstones cleared} accumulate
// in its row of the call's result array, and k_gc_end_multi (one thread per map)
// lowers the map's device count by the deletions and leaves the count in row[2].
#define GF_GC_MULTI 32u
struct GcMap {
    gf_htab_desc d;
    uint32_t *bits;                     // the map's cluster-start bits (Map::d_gcbits)
    unsigned long long *res;            // its result row: deleted, tombstones cleared, count after, 0
    uint32_t mode, lt_off;
};
struct GcBatch { GcMap m[GF_GC_MULTI]; uint32_t t0[GF_GC_MULTI + 1]; uint32_t n; };
static_assert(sizeof(GcBatch) + 64 <= 4096, "the maps travel in the kernel arguments");
// The map of tile t (t < B.t0[B.n]); k: the block's previous answer (tiles only grow).
__device__ __forceinline__ uint32_t gc_tile_map(const GcBatch &B, uint32_t t, uint32_t k) {
    while (t >= B.t0[k + 1]) k++;
    return k;
}
__global__ __launch_bounds__(BLOCK) void k_gc_starts_multi(GcBatch B) {
    uint32_t k = 0;
    for (uint32_t t = blockIdx.x; t < B.t0[B.n]; t += gridDim.x) {
        k = gc_tile_map(B, t, k);
        const GcMap &M = B.m[k];
        const uint64_t w = (uint64_t)(t - B.t0[k]) * BLOCK + threadIdx.x;
        if (w < (M.d.mask + 1 + 31) / 32) gc_starts_word(M.d, M.bits, w);
    }
}
__global__ __launch_bounds__(BLOCK) void k_gc_clusters_multi(GcBatch B, uint32_t filter_time) {
    const GcCut cut{filter_time, filter_time, 1u, 0u};      // lifetime < filter_time
    uint32_t k = 0;
    for (uint32_t t = blockIdx.x; t < B.t0[B.n]; t += gridDim.x) {
        k = gc_tile_map(B, t, k);
        const GcMap &M = B.m[k];
        const uint64_t w = (uint64_t)(t - B.t0[k]) * BLOCK + threadIdx.x;
        if (w >= (M.d.mask + 1 + 31) / 32) continue;
        const uint32_t vstride = M.d.vals ? (M.d.sstride ? M.d.sstride : M.d.vsz) : 0u;
        uint32_t dead = 0, tombs = 0;
        gc_clusters_word(M.d, M.mode, M.lt_off, cut, vstride, M.bits, w, dead, tombs);
        if (dead) atomicAdd(&M.res[0], (unsigned long long)dead);
        if (tombs) atomicAdd(&M.res[1], (unsigned long long)tombs);
    }
}
__global__ void k_gc_end_multi(GcBatch B) {
    if (threadIdx.x >= B.n) return;
    const GcMap &M = B.m[threadIdx.x];
    const unsigned long long dead = M.res[0];
    const uint32_t c = *M.d.count;
    const uint32_t after = (unsigned long long)c >= dead ? c - (uint32_t)dead : 0u;
    *M.d.count = after;
    M.res[2] = after;
}

// ---- cilium_proxy{4,6} sweeps (gf_proxy_gc / gf_proxy_cleanup_port; pkg/maps/proxymap:
// gc / gc6, cleanupIPv{4,6}Redirects).  The same two-step sweep over the proxy maps'
// own layout and hash (GF_HASH_PLAIN, the slot geometry of hdesc()): k_gc_starts marks
// the cluster starts, k_px_gc walks each cluster with one lane.  The predicate is a
// launch argument: by lifetime (the last u32 of proxy{4,6}_tbl_value, strictly below
// the cutoff) or by port (key.dport == arg as stored, and key.nexthdr == 6).
enum { GF_PXGC_LIFETIME = 0, GF_PXGC_PORT = 1 };
struct PxGcPred {
    uint32_t mode;              // GF_PXGC_*
    uint32_t arg;               // the cutoff (seconds) or the raw be16 port
    uint32_t off;               // value offset of lifetime / key offset of dport
    uint32_t nh_off;            // key offset of nexthdr (port mode)
};
struct PxGcDev {                // per call context, device memory
    GcCut on;                   // k_gc_starts' switch (active = 1)
    unsigned long long res[2];  // entries deleted, tombstones cleared
};
__device__ __forceinline__ bool px_gc_kill(const gf_htab_desc &d, uint64_t j, const PxGcPred &P) {
    if (P.mode == GF_PXGC_LIFETIME) return *reinterpret_cast<const uint32_t *>(ht_val(d, j) + P.off) < P.arg;
    const uint8_t *k = d.slots + j * d.slot_size;
    return *reinterpret_cast<const uint16_t *>(k + P.off) == P.arg && k[P.nh_off] == 6;
}
__global__ __launch_bounds__(BLOCK) void k_px_gc(gf_htab_desc d, PxGcPred P, const uint32_t *bits, unsigned long long *res) {
    const uint64_t nw = (d.mask + 1 + 31) / 32;
    uint32_t dead = 0, tombs = 0;
    for (uint64_t w = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; w < nw; w += (uint64_t)gridDim.x * blockDim.x) {
        uint32_t m = bits[w];
        while (m) {
            const int k = __builtin_ctz(m);
            m &= m - 1;
            uint64_t j = w * 32 + k;
            // as in k_gc_clusters: nothing moves until this walk has emptied a slot of the
            // cluster; n bounds the walk by the table (a cluster ends at an EMPTY slot)
            bool hole = false;
            for (uint64_t n = 0; n <= d.mask; n++, j = (j + 1) & d.mask) {
                uint8_t *sl = d.slots + j * d.slot_size;
                const uint32_t st = sl[d.ksz];
                if (st == GF_SLOT_EMPTY) break;
                if (st == GF_SLOT_TOMB || st == GF_SLOT_FREE) {
                    sl[d.ksz] = GF_SLOT_EMPTY;
                    tombs++;
                    hole = true;
                } else if (px_gc_kill(d, j, P)) {
                    sl[d.ksz] = GF_SLOT_EMPTY;
                    dead++;
                    hole = true;
                } else if (hole) {
                    uint32_t kw[6];                             // 22 B at most (gf_proxy_* checks the sizes)
                    for (uint32_t q = 0; q < 6; q++) kw[q] = 0;
                    for (uint32_t q = 0; q < d.ksz; q += 4) {   // slots are 16-B aligned
                        const uint32_t x = *reinterpret_cast<const uint32_t *>(sl + q);
                        kw[q >> 2] = d.ksz - q >= 4 ? x : (x & ((1u << (8 * (d.ksz - q))) - 1u));
                    }
                    const uint64_t home = gf_home_slot(gf_key_hash(kw, d.ksz, GF_HASH_PLAIN), d.mask, d.slot_size);
                    for (uint64_t p = home; p != j; p = (p + 1) & d.mask) {
                        if (d.slots[p * d.slot_size + d.ksz] == GF_SLOT_EMPTY) { gc_move(d, j, p, 0u); break; }
                    }
                }
            }
        }
    }
    if (dead) atomicAdd(&res[0], (unsigned long long)dead);
    if (tombs) atomicAdd(&res[1], (unsigned long long)tombs);
}

// ---- LRU stand-in (CT maps are BPF_MAP_TYPE_LRU_HASH, bpf/bpf_lxc.c:53-75;
// ctmap.go:38-39).  The kernel never fails an LRU insert: it evicts from per-CPU
// LRU lists, taking entries off the tail of an inactive list it keeps about as
// long as the active one (kernel/bpf/bpf_lru_list.c, not in /root/reference) — in
// effect from the older half of the entries, in an order nothing reproduces.
// Here an LRU CT map may exceed max_entries inside a batch (the slot array has
// room); at the end of every classify call that inserts into it, once the device
// count exceeds the high-water mark HW = max_entries - max_entries / 8, a
// deterministic *hand* evicts (the oracle restates it, o_ct_lru_evict):
//  * age key of an entry: 0 if its last use (ct_last_use) lies before time 0,
//    else closing entries (rx_closing | tx_closing) in [0, 65536) and the others
//    in [65536, 131072), each by last use in one-second bins relative to now (bin
//    0 = last used 65535 s or more ago);
//  * home line of an entry: its key's home slot in this table (gf_home_slot of the
//    CT hash) / slots per 128-B line; NL lines in all;
//  * the sample: the entries homed in the SL lines from where the hand stands (SL
//    = NL when NL <= 65536, else max(65536, NL >> 10)), the lines it passes next.  K = the smallest age key covering half of
//    the sample (its older half is eligible); es = the sample entries with age key
//    <= K.  A window that holds no entry (only keys chosen to avoid those lines)
//    is replaced by the whole table (SL = NL);
//  * the lines for q entries: ceil(q * SL / es);
//  * round 0 (count > HW): q = count - HW; round 1 (only while count >
//    max_entries): q = count - HW again, for what round 0's estimate left; round 2
//    (only while count > max_entries still): the rest of the table.  Each round
//    passes its lines (at most NL - the lines already passed) from where the hand
//    stands and deletes every entry with age key <= K homed in them.
// A map that runs at HW deletes in each call about what the call inserted, so
// the work per call follows the call's inserts, not the table; the count is back
// at <= max_entries after every call unless fewer than count - max_entries
// entries are eligible in the whole table (documented bound, include/gpuflow.h).
// A deleted slot turns EMPTY when every slot after it up to the end of its probe
// cluster is gone too (the probe invariant holds), else FREE (claimed by later
// device inserts, gf_common.h); tombstones the hand passes are cleared the same
// way.  Key bytes of the cleared slots are zeroed.  Every eviction is logged
// (gf_ct_evict_log: batch number, now, K, the hand's first line, lines passed,
// entries deleted).
#define GF_LRU_BINS 65536u
#define GF_LRU_LOGCAP 4096u
#define GF_LRU_SAMPLE_SHIFT 10
#define GF_LRU_SAMPLE_MIN 65536ull
#define GF_LRU_ROUNDS 3u
#define GF_LRU_HT 256u                  // k_lru_hand block
#define GF_LRU_CHUNK 1024u              // k_lru_hand: slots a block decides together (CT6; CT4 twice that)
struct LruLog { uint32_t seq, now, age_cut, pad; unsigned long long hand, lines, evicted; };
#define GF_LRU_GROUPS (2u * GF_LRU_BINS / 64u)
struct LruDev {
    uint32_t hist[2 * GF_LRU_BINS];     // the sample's age histogram
    uint32_t coarse[GF_LRU_GROUPS];     // its sums per group of 64 bins (k_lru_plan reads these first)
    GcCut cut;                          // gf_ct_gc (k_gc_*)
    unsigned long long res[2];          // gf_ct_gc: entries deleted, tombstones cleared
    uint32_t flag;                      // this call evicts (count > HW)
    uint32_t K;                         // age keys [0, K] are eligible
    unsigned long long es;              // eligible sample entries (0: empty sample, age-blind)
    unsigned long long hand;            // the hand's next home line (kept across calls)
    unsigned long long cnt0;            // the count when this call's eviction began
    unsigned long long sl;              // the lines the sample covered (the window, or the table)
    uint32_t wide, pad1;                // the window held no entry: sample the whole table
    unsigned long long kills[GF_LRU_ROUNDS];   // entries deleted by each round
    unsigned long long cleared;         // tombstones / FREE slots rewritten (diagnostics)
    uint32_t nlog, pad;
    LruLog log[GF_LRU_LOGCAP];
};
// The sampled home lines of a table of nl lines.
__host__ __device__ __forceinline__ uint64_t lru_sample_lines(uint64_t nl) {
    if (nl <= GF_LRU_SAMPLE_MIN) return nl;
    const uint64_t s = nl >> GF_LRU_SAMPLE_SHIFT;
    return s > GF_LRU_SAMPLE_MIN ? s : GF_LRU_SAMPLE_MIN;
}
__host__ __device__ __forceinline__ unsigned long long lru_high_water(uint32_t max_entries) {
    return (unsigned long long)(max_entries - max_entries / 8u);
}
// Round r of this call: the hand's first line and the lines it passes, from the
// call's state (count at the start, K / es, the earlier rounds' deletions).  Every
// block of a round's launches computes the same values; nothing is written.
struct LruRound { unsigned long long h0, lines; };
__device__ __forceinline__ LruRound lru_round(const LruDev *L, uint32_t r, uint32_t max_entries, uint64_t nl) {
    const unsigned long long hw = lru_high_water(max_entries), es = L->es, sl = L->sl;
    unsigned long long c = L->cnt0, passed = 0, h = L->hand;
    LruRound o{h, 0ull};
    if (!L->flag) return o;
    for (uint32_t j = 0; j <= r; j++) {
        if (j) c -= L->kills[j - 1];
        unsigned long long ln = 0;
        if ((j == 0 ? c > hw : c > (unsigned long long)max_entries) && passed < nl) {
            if (j + 1 < GF_LRU_ROUNDS) {
                const unsigned long long q = c - hw;
                ln = es ? (q * sl + es - 1) / es : nl;  // es >= 1: the sample holds entries
                if (ln > nl - passed) ln = nl - passed;
            } else {
                ln = nl - passed;
            }
        }
        if (j == r) { o.h0 = h; o.lines = ln; return o; }
        h = (h + ln) % nl;
        passed += ln;
    }
    return o;
}
__device__ __forceinline__ uint32_t lru_age_key(uint32_t lt, uint32_t fl, uint32_t now) {
    const long long lu = ct_last_use(lt, fl);
    if (lu < 0) return 0u;
    long long b = lu - ((long long)now - (long long)(GF_LRU_BINS - 1));
    b = b < 0 ? 0 : (b > (long long)(GF_LRU_BINS - 1) ? (long long)(GF_LRU_BINS - 1) : b);
    return ((fl & (F_RX_CLOSING | F_TX_CLOSING)) ? 0u : GF_LRU_BINS) + (uint32_t)b;
}
// One CT slot as the eviction pass reads it.  KIND 1: the CT v4 slot (32 B: key
// 14, state at 14, hot value at 16 with the lifetime first) as two 16-B loads;
// KIND 2: the CT v6 slot (64 B: key 40, state at 40, hot value at 48) as four.
template <int KIND>
struct LruSlot {
    static constexpr uint32_t SZ = KIND == 2 ? 64u : 32u, SPL = 128u / SZ, KW = KIND == 2 ? 10 : 4;
    uint32_t kw[KW];
    uint32_t st = GF_SLOT_EMPTY, lt = 0, fl = 0;
    // plain loads: the eviction passes stream GBs of slots per call, but nontemporal loads
    // (to spare the next launch's policy maps and hot CT lines in L2 / MALL) made the hand
    // 7-12 % slower and left the next k_ing_groups unchanged (same-box A/B, r6e)
    __device__ __forceinline__ static uint4 ld(const uint8_t *p) { return gload<uint4>(p); }
    __device__ __forceinline__ void load(const gf_htab_desc &d, uint64_t i) {
        const uint8_t *p = d.slots + i * SZ;
        if constexpr (KIND == 2) {
            const uint4 a = ld(p), b = ld(p + 16), c = ld(p + 32), e = ld(p + 48);
            kw[0] = a.x; kw[1] = a.y; kw[2] = a.z; kw[3] = a.w; kw[4] = b.x; kw[5] = b.y; kw[6] = b.z; kw[7] = b.w;
            kw[8] = c.x; kw[9] = c.y;
            st = c.z & 0xffu; lt = e.x; fl = e.y & 0xffffu;
        } else {
            const uint4 a = ld(p), b = ld(p + 16);
            kw[0] = a.x; kw[1] = a.y; kw[2] = a.z; kw[3] = a.w & 0xffffu;
            st = (a.w >> 16) & 0xffu; lt = b.x; fl = b.y & 0xffffu;
        }
    }
    __device__ __forceinline__ uint64_t home_line(const gf_htab_desc &d, uint32_t mode) const {
        return gf_home_slot(gf_key_hash(kw, KIND == 2 ? 40u : 14u, mode), d.mask, SZ) / SPL;
    }
};
// A deleted / cleared slot: key bytes zeroed, state EMPTY or FREE (16-B stores).
template <int KIND>
__device__ __forceinline__ void lru_clear_slot(const gf_htab_desc &d, uint64_t j, uint32_t st) {
    uint8_t *p = d.slots + j * LruSlot<KIND>::SZ;
    if constexpr (KIND == 2) {
        gstore<uint4>(p + 32, make_uint4(0u, 0u, st, 0u));
        gstore<uint4>(p, make_uint4(0u, 0u, 0u, 0u));
        gstore<uint4>(p + 16, make_uint4(0u, 0u, 0u, 0u));
    } else {
        gstore<uint4>(p, make_uint4(0u, 0u, 0u, st << 16));
    }
}
// The chain after a classify call: k_lru_sample, k_lru_plan, k_lru_hand x 2 per
// round (GF_LRU_ROUNDS), k_lru_end.  Each launch exits at once unless the count
// exceeds HW (and a round's, unless the round passes lines).  The histogram is zero
// between calls (cleared by k_lru_plan after its scan; zero at allocation).
// Age histogram of the sample: wave-aggregated (a wave's entries mostly share a
// bin), then counted per block in LDS and flushed with one global add per
// non-zero bin.  The last GF_LRU_WIN seconds of each class are counted directly
// (one LDS slot per bin, no collisions): a steady stream's live entries were all
// last used within its flows' lifetimes.  Older bins go through a block-local
// LDS cache: a 64-bit {bin, count} word per line (Fibonacci-hashed), updated by
// CAS; a bin that misses takes the line over and flushes the previous bin's
// count with one global add.  (An XOR-folded index once mapped a closing bin and
// the non-closing bin 32 s from it to one line: every wave alternated them and
// sent a global add to a few hot addresses.)
#define GF_LRU_LDS 2048u
#define GF_LRU_WIN 4096u
#define GF_LRU_HB 1024u                 // k_lru_sample block: 16 waves share the LDS bins
// One histogram add; its group's sum goes to the block's LDS copy of the sums
// (flushed once per block: a sample's entries fall in a few groups, whose global
// words every block would otherwise hit for each of its bins).
__device__ __forceinline__ void lru_hist_put(LruDev *L, uint32_t *cg, uint32_t bin, uint32_t c) {
    atomicAdd(&L->hist[bin], c);
    atomicAdd(&cg[bin >> 6], c);
}
// key: the entry's age key, ~0u for none.  Wave-uniform call.
__device__ __forceinline__ void lru_hist_add(LruDev *L, unsigned long long *line, uint32_t *win, uint32_t *cg,
                                             uint32_t key) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t kb = key & (GF_LRU_BINS - 1u);
    const bool inwin = key != ~0u && kb >= GF_LRU_BINS - GF_LRU_WIN;
    if (inwin) atomicAdd(&win[(key >> 16) * GF_LRU_WIN + kb - (GF_LRU_BINS - GF_LRU_WIN)], 1u);
    uint64_t rem = __ballot(key != ~0u && !inwin);
    while (rem) {
        const uint32_t lead = (uint32_t)__ffsll((unsigned long long)rem) - 1u;
        const uint32_t k = __shfl(key, (int)lead);
        const uint64_t m = __ballot(key == k) & rem;
        if (lane == lead) {
            const uint32_t n = (uint32_t)__popcll(m), h = (k * 0x9E3779B1u) >> (32 - 11);
            unsigned long long cur = line[h];
            for (;;) {
                const uint32_t ck = (uint32_t)(cur >> 32);
                const unsigned long long want = ck == k ? cur + n : (((unsigned long long)k << 32) | n);
                const unsigned long long seen = atomicCAS(&line[h], cur, want);
                if (seen == cur) {
                    if (ck != k && ck != ~0u && (uint32_t)cur) lru_hist_put(L, cg, ck, (uint32_t)cur);
                    break;
                }
                cur = seen;
            }
        }
        rem &= ~m;
    }
}
// The sample: the sl home lines just ahead of the hand (the lines it passes next,
// so their density is the one its rounds are planned with; the whole table when
// sl = nl): slots [hand * SPL, (hand + sl) * SPL) mod NS and the rest of the probe
// cluster running past them (entries homed in the window; one wave walks it, at
// most to where the window starts again).
// wide: the whole table (launched after k_lru_plan found the window empty).
template <int KIND>
__device__ __forceinline__ void lru_sample_body(const gf_htab_desc &d, uint32_t mode, uint32_t now, LruDev *L,
                                                uint64_t sl, uint32_t max_entries, uint32_t wide) {
    if (wide ? !L->wide : (unsigned long long)*d.count <= lru_high_water(max_entries)) return;
    __shared__ unsigned long long line[GF_LRU_LDS];    // bin << 32 | count; bin ~0 = empty
    __shared__ uint32_t win[2 * GF_LRU_WIN];           // class * WIN + bin - (BINS - WIN)
    __shared__ uint32_t cg[GF_LRU_GROUPS];             // the block's group sums
    for (uint32_t k = threadIdx.x; k < GF_LRU_LDS; k += blockDim.x) line[k] = 0xffffffff00000000ull;
    for (uint32_t k = threadIdx.x; k < 2 * GF_LRU_WIN; k += blockDim.x) win[k] = 0;
    for (uint32_t k = threadIdx.x; k < GF_LRU_GROUPS; k += blockDim.x) cg[k] = 0;
    __syncthreads();
    constexpr uint32_t SPL = LruSlot<KIND>::SPL;
    const uint64_t ns = d.mask + 1, nl = ns / SPL;
    if (wide) sl = nl;
    const uint64_t n = sl * SPL, h0 = sl >= nl ? 0 : L->hand, P0 = h0 * SPL;
    auto in_window = [&](const LruSlot<KIND> &s) { return (s.home_line(d, mode) + nl - h0) % nl < sl; };
    for (uint64_t b0 = (uint64_t)blockIdx.x * GF_LRU_HB; b0 < n; b0 += (uint64_t)gridDim.x * GF_LRU_HB) {  // uniform trips
        const uint64_t i = b0 + threadIdx.x;
        uint32_t key = ~0u;
        if (i < n) {
            LruSlot<KIND> s;
            s.load(d, (P0 + i) & d.mask);
            if (s.st == GF_SLOT_FULL && in_window(s)) key = lru_age_key(s.lt, s.fl, now);
        }
        lru_hist_add(L, line, win, cg, key);
    }
    if (blockIdx.x == 0 && threadIdx.x < 64 && n < ns) {
        for (uint64_t q = n;; q += 64) {
            const uint64_t i = q + threadIdx.x;
            LruSlot<KIND> s;
            if (i < ns) s.load(d, (P0 + i) & d.mask);
            const uint64_t em = __ballot(s.st == GF_SLOT_EMPTY);
            const uint32_t stop = em ? (uint32_t)__ffsll((unsigned long long)em) - 1u : 64u;
            uint32_t key = ~0u;
            if (threadIdx.x < stop && s.st == GF_SLOT_FULL && in_window(s)) key = lru_age_key(s.lt, s.fl, now);
            lru_hist_add(L, line, win, cg, key);
            if (em || q + 64 >= ns) break;
        }
    }
    __syncthreads();
    for (uint32_t k = threadIdx.x; k < GF_LRU_LDS; k += blockDim.x) {
        const unsigned long long v = line[k];
        if ((uint32_t)(v >> 32) != ~0u && (uint32_t)v) lru_hist_put(L, cg, (uint32_t)(v >> 32), (uint32_t)v);
    }
    for (uint32_t k = threadIdx.x; k < 2 * GF_LRU_WIN; k += blockDim.x)
        if (win[k]) lru_hist_put(L, cg, (k / GF_LRU_WIN) * GF_LRU_BINS + GF_LRU_BINS - GF_LRU_WIN + k % GF_LRU_WIN, win[k]);
    __syncthreads();
    for (uint32_t k = threadIdx.x; k < GF_LRU_GROUPS; k += blockDim.x)
        if (cg[k]) atomicAdd(&L->coarse[k], cg[k]);
}
template <int KIND>
__global__ __launch_bounds__(GF_LRU_HB) void k_lru_sample(gf_htab_desc d, uint32_t mode, uint32_t now, LruDev *L,
                                                          uint64_t sl, uint32_t max_entries, uint32_t wide) {
    lru_sample_body<KIND>(d, mode, now, L, sl, max_entries, wide);
}
// K and es from the sample's histogram, the count the call starts from, and the
// histogram cleared for the next call (one block).
// wide = 0: the window's sample; an empty one (sl < nl) sets L->wide for the
// whole-table sample and its plan (wide = 1) instead of planning.
__device__ __forceinline__ void lru_plan_body(const uint32_t *count, uint32_t max_entries, LruDev *L, uint64_t sl,
                                              uint64_t nl, uint32_t wide) {
    const uint32_t c = *count;
    const uint32_t t = threadIdx.x;
    if (wide) {
        if (!L->wide) return;
        sl = nl;
    } else if ((unsigned long long)c <= lru_high_water(max_entries)) {
        if (t == 0) L->flag = 0u;
        return;
    }
    // the 2048 group sums (two per thread), a block scan, then one wave finds the
    // median's bin among its group's 64; only the groups that hold entries are cleared
    constexpr uint32_t NB = 2 * GF_LRU_BINS;
    __shared__ unsigned long long part[1024];
    __shared__ uint32_t s_k, s_g;
    __shared__ unsigned long long s_es, s_before;
    const uint32_t g0 = L->coarse[2 * t], g1 = L->coarse[2 * t + 1];
    if (t == 0) { s_k = NB - 1; s_es = 0; s_g = ~0u; s_before = 0; }
    {                                                   // inclusive scan: in each wave, then over the 16 waves
        const uint32_t lane = t & 63u, wv = t >> 6;
        unsigned long long v = (unsigned long long)g0 + g1;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned long long u = __shfl_up(v, o);
            if (lane >= (uint32_t)o) v += u;
        }
        __shared__ unsigned long long wsum[16];
        if (lane == 63) wsum[wv] = v;
        __syncthreads();
        unsigned long long off = 0;
        for (uint32_t q = 0; q < wv; q++) off += wsum[q];
        part[t] = v + off;
        __syncthreads();
    }
    const unsigned long long total = part[1023], need = (total + 1) / 2, before = t ? part[t - 1] : 0ull;
    if (!total && sl < nl) {                            // no entry in the window (histogram still all zero)
        if (t == 0) { L->wide = 1u; L->flag = 0u; }
        return;
    }
    if (total && before < need && part[t] >= need) {    // the median lies in group 2t or 2t + 1
        const bool first = before + g0 >= need;
        s_g = first ? 2 * t : 2 * t + 1;
        s_before = first ? before : before + g0;
    }
    __syncthreads();
    if (t < 64 && s_g != ~0u) {                          // wave 0: the median group's bins, one per lane
        const uint32_t v = L->hist[s_g * 64u + t];
        uint32_t inc = v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t u = __shfl_up(inc, o);
            if (t >= (uint32_t)o) inc += u;
        }
        const uint64_t hit = __ballot(s_before + inc >= need);
        if (t == (uint32_t)__ffsll((unsigned long long)hit) - 1u) { s_k = s_g * 64u + t; s_es = s_before + inc; }
    }
    __syncthreads();
    // clear for the next sample: the bins of the groups that hold entries, and the sums
    for (uint32_t q = 0; q < 2; q++) {
        const uint32_t g = 2 * t + q;
        if (!(q ? g1 : g0)) continue;
        uint4 *hb = reinterpret_cast<uint4 *>(L->hist + g * 64u);
#pragma unroll
        for (uint32_t k = 0; k < 16; k++) hb[k] = make_uint4(0u, 0u, 0u, 0u);
        L->coarse[g] = 0u;
    }
    if (t == 0) {
        L->K = s_k; L->es = s_es; L->cnt0 = c; L->sl = sl; L->wide = 0u; L->flag = 1u; L->cleared = 0;
        for (uint32_t r = 0; r < GF_LRU_ROUNDS; r++) L->kills[r] = 0;
    }
}
__global__ __launch_bounds__(1024) void k_lru_plan(const uint32_t *count, uint32_t max_entries, LruDev *L, uint64_t sl,
                                                   uint64_t nl, uint32_t wide) {
    lru_plan_body(count, max_entries, L, sl, nl, wide);
}
// The hand over this round's lines: the slots from the first line's first slot,
// lines * SPL of them, in chunks (GF_LRU_CHUNK slots, twice that for CT4), plus the cluster running past
// the last one (entries homed in the range).  Launched twice, PAR = 0 for the
// even chunks and 1 for the odd ones: a chunk's last slots turn EMPTY only if the
// slots after it, up to the cluster's end, are all gone too, which the block
// reads from the next chunk (at most one chunk ahead, else it keeps them FREE) —
// untouched in the even launch, final in the odd one, so no read races a write.
// The slots past the last chunk are read and written by its block alone (there
// deleted entries turn FREE).  Codes: 0 EMPTY, 1 kept, 2 deleted now, 3 a
// tombstone or FREE slot (cleared).
template <int KIND, int PAR>
__device__ __forceinline__ void lru_hand_body(const gf_htab_desc &d, uint32_t mode, uint32_t now, LruDev *L,
                                              uint64_t nl, uint64_t sl, uint32_t max_entries, uint32_t round) {
    if (!L->flag) return;
    const LruRound R = lru_round(L, round, max_entries, nl);
    const unsigned long long lines = R.lines;
    if (!lines) return;
    using S = LruSlot<KIND>;
    // slots a block decides together: 8 per thread for the 32-B CT4 slots, 4 for the
    // 64-B CT6 slots (the same 64 KB of loads in flight per block)
    constexpr uint32_t CH = KIND == 2 ? GF_LRU_CHUNK : 2 * GF_LRU_CHUNK, U = CH / GF_LRU_HT;
    const uint32_t K = L->K;
    const unsigned long long h0 = R.h0;
    const uint64_t ns = d.mask + 1, P0 = h0 * S::SPL, NP = lines * S::SPL;
    const bool whole = NP >= ns;
    const uint64_t nch = (NP + CH - 1) / CH;
    __shared__ uint8_t code[2 * GF_LRU_CHUNK];
    __shared__ uint32_t s_ef, s_kills, s_clr;
    auto code_of = [&](const S &s) -> uint32_t {
        if (s.st == GF_SLOT_EMPTY) return 0u;
        if (s.st == GF_SLOT_TOMB || s.st == GF_SLOT_FREE) return 3u;
        if (s.st != GF_SLOT_FULL || lru_age_key(s.lt, s.fl, now) > K) return 1u;
        const uint64_t hl = s.home_line(d, mode);
        return (hl + nl - h0) % nl < lines ? 2u : 1u;
    };
    if (threadIdx.x == 0) { s_kills = 0; s_clr = 0; }
    uint32_t kills = 0, clr = 0;
    const uint32_t lane = threadIdx.x & 63u;
    for (uint64_t c = 2 * (uint64_t)blockIdx.x + PAR; c < nch; c += 2 * (uint64_t)gridDim.x) {
        const uint64_t base = c * CH;
        const uint32_t cnt = (uint32_t)(NP - base < CH ? NP - base : CH);
        const bool last = base + cnt == NP;
        uint32_t mine[U], ost[U];
        // wave 0 also loads the first 64 slots after the chunk with the chunk's own
        // loads (at low load they decide the chunk's trailing run): one round trip
        // less per chunk.  Nothing writes them during this launch before wave 0 reads
        // them below (the next chunk is the other launch's, and past the last chunk
        // only this block writes, after reading).
        S la;
        const bool look = threadIdx.x < 64 && !(last && whole);
        const uint64_t o0 = base + cnt + lane;
        if (look && o0 < ns) la.load(d, (P0 + o0) & d.mask);
#pragma unroll
        for (uint32_t u = 0; u < U; u++) {
            const uint32_t off = u * GF_LRU_HT + threadIdx.x;
            mine[u] = 1u; ost[u] = GF_SLOT_FULL;
            if (off < cnt) {
                S s;
                s.load(d, (P0 + base + off) & d.mask);
                mine[u] = code_of(s);
                ost[u] = s.st;
                code[off] = (uint8_t)mine[u];
            }
        }
        __syncthreads();
        if (threadIdx.x < 64) {                          // wave 0: the slots after the chunk
            bool ef = false, decided = false;
            if (look) {
                for (uint64_t q = 0;; q += 64) {
                    if (!last && q >= CH) break;                           // undecided: the chunk's run stays FREE
                    const uint64_t o = base + cnt + q + lane;              // offset from P0
                    uint32_t cd = 0;
                    if (o < ns) {                                          // never back into the range
                        const uint64_t j = (P0 + o) & d.mask;
                        if (q) la.load(d, j);
                        cd = code_of(la);
                        if (last && cd == 2) { lru_clear_slot<KIND>(d, j, GF_SLOT_FREE); kills++; }
                    }
                    const uint64_t stop_m = __ballot(cd <= 1u);
                    if (!decided && stop_m) {
                        ef = __shfl(cd, (int)((uint32_t)__ffsll((unsigned long long)stop_m) - 1u)) == 0u;
                        decided = true;
                    }
                    if (!last && decided) break;
                    if (last && __ballot(cd == 0u)) break;                 // the cluster past the range ends
                }
            }
            if (lane == 0) s_ef = decided && ef ? 1u : 0u;
        }
        __syncthreads();
        const bool ef = s_ef != 0;
#pragma unroll
        for (uint32_t u = 0; u < U; u++) {
            const uint32_t off = u * GF_LRU_HT + threadIdx.x;
            if (off >= cnt || mine[u] < 2u) continue;
            bool to_empty = ef;
            for (uint32_t k = off + 1; k < cnt; k++) {
                const uint32_t x = code[k];
                if (x <= 1u) { to_empty = x == 0u; break; }
            }
            const uint32_t nst = to_empty ? GF_SLOT_EMPTY : GF_SLOT_FREE;
            if (mine[u] == 2u) kills++;
            else if (ost[u] != nst) clr++;
            if (mine[u] == 2u || ost[u] != nst) lru_clear_slot<KIND>(d, (P0 + base + off) & d.mask, nst);
        }
        __syncthreads();                                 // code[] is the next chunk's
    }
    if (kills) atomicAdd(&s_kills, kills);
    if (clr) atomicAdd(&s_clr, clr);
    __syncthreads();
    if (threadIdx.x == 0) {
        if (s_kills) atomicAdd(&L->kills[round], (unsigned long long)s_kills);
        if (s_clr) atomicAdd(&L->cleared, (unsigned long long)s_clr);
    }
}
template <int KIND, int PAR>
__global__ __launch_bounds__(GF_LRU_HT) void k_lru_hand(gf_htab_desc d, uint32_t mode, uint32_t now, LruDev *L,
                                                        uint64_t nl, uint64_t sl, uint32_t max_entries, uint32_t round) {
    lru_hand_body<KIND, PAR>(d, mode, now, L, nl, sl, max_entries, round);
}
// After the last round: the count, the hand, the log (hcount: the count for the
// host's bound, pinned host memory, may be null).
__device__ __forceinline__ void lru_end_body(uint32_t *count, uint32_t seq, uint32_t now, LruDev *L,
                                             uint32_t max_entries, uint64_t nl, uint32_t *hcount) {
    if (!L->flag) {
        if (hcount) *hcount = *count;
        return;
    }
    unsigned long long killed = 0, lines = 0;
    for (uint32_t r = 0; r < GF_LRU_ROUNDS; r++) {
        lines += lru_round(L, r, max_entries, nl).lines;
        killed += L->kills[r];
    }
    *count = (uint32_t)(*count - killed);
    const uint32_t n = L->nlog;
    if (n < GF_LRU_LOGCAP) {
        LruLog &g = L->log[n];
        g.seq = seq; g.now = now; g.age_cut = L->K; g.pad = 0;
        g.hand = L->hand; g.lines = lines; g.evicted = killed;
    }
    L->nlog = n + 1;
    L->hand = (L->hand + lines) % nl;
    L->flag = 0;
    if (hcount) *hcount = *count;
}
__global__ void k_lru_end(uint32_t *count, uint32_t seq, uint32_t now, LruDev *L, uint32_t max_entries, uint64_t nl,
                          uint32_t *hcount) {
    lru_end_body(count, seq, now, L, max_entries, nl, hcount);
}

// The same chain over several maps of one slot kind at once (per-endpoint CT maps,
// the ConntrackLocal option): one launch per phase for up to GF_LRU_MULTI maps, each
// block running every map's share in turn (the plan and the end: one block / one
// thread per map).  The maps travel in the kernel arguments.
#define GF_LRU_MULTI 32u
struct LruMap {
    gf_htab_desc d;
    LruDev *L;
    uint64_t nl, sl;
    uint32_t mode, max_entries, seq, pad;
    uint32_t *hcount;
    unsigned long long *stamp;          // multi-map pass: seq << 32 | count after the pass (pinned), or null
};
struct LruBatch { LruMap m[GF_LRU_MULTI]; uint32_t n; };
static_assert(GF_LRU_MULTI <= 32, "lru_active keeps one bit per map in a 32-bit mask");
static_assert(sizeof(LruBatch) + 64 <= 4096, "the maps travel in the kernel arguments");
// The batch's maps a phase has work for, read by one lane per map at once (a block
// would otherwise pay one dependent round trip per map): what 0 = over the high-water
// mark (the sample; wide: the window was empty), 1 = evicting this call (the hand).
__device__ __forceinline__ uint32_t lru_active(const LruBatch &B, uint32_t what, uint32_t wide) {
    __shared__ uint32_t s_mask;
    if (threadIdx.x < 64) {
        bool a = false;
        if (threadIdx.x < B.n) {
            const LruMap &M = B.m[threadIdx.x];
            if (what) a = M.L->flag != 0u;
            else a = wide ? M.L->wide != 0u : (unsigned long long)*M.d.count > lru_high_water(M.max_entries);
        }
        const uint64_t b = __ballot(a);
        if (threadIdx.x == 0) s_mask = (uint32_t)b;
    }
    __syncthreads();
    return s_mask;
}
template <int KIND>
__global__ __launch_bounds__(GF_LRU_HB) void k_lru_sample_multi(LruBatch B, uint32_t now, uint32_t wide) {
    const uint32_t act = lru_active(B, 0u, wide);
    for (uint32_t k = 0; k < B.n; k++) {
        if (!((act >> k) & 1u)) continue;
        const LruMap &M = B.m[k];
        lru_sample_body<KIND>(M.d, M.mode, now, M.L, M.sl, M.max_entries, wide);
        __syncthreads();                                // the LDS bins are the next map's
    }
}
__global__ __launch_bounds__(1024) void k_lru_plan_multi(LruBatch B, uint32_t wide) {
    const LruMap &M = B.m[blockIdx.x];
    lru_plan_body(M.d.count, M.max_entries, M.L, M.sl, M.nl, wide);
}
template <int KIND, int PAR>
__global__ __launch_bounds__(GF_LRU_HT) void k_lru_hand_multi(LruBatch B, uint32_t now, uint32_t round) {
    const uint32_t act = lru_active(B, 1u, 0u);
    for (uint32_t k = 0; k < B.n; k++) {
        if (!((act >> k) & 1u)) continue;
        const LruMap &M = B.m[k];
        lru_hand_body<KIND, PAR>(M.d, M.mode, now, M.L, M.nl, M.sl, M.max_entries, round);
        __syncthreads();                                // code[] and the block's counts are the next map's
    }
}
__global__ void k_lru_end_multi(LruBatch B, uint32_t now) {
    if (threadIdx.x >= B.n) return;
    const LruMap &M = B.m[threadIdx.x];
    lru_end_body(M.d.count, M.seq, now, M.L, M.max_entries, M.nl, M.hcount);
    if (M.stamp) *M.stamp = ((unsigned long long)M.seq << 32) | *M.d.count;
}

// ================================================================ drop notifications
// send_drop_notify / __send_drop_notify (bpf/lib/drop.h:47-107, DROP_NOTIFY): one
// struct drop_notify (32 B, pkg/monitor DropNotify) + up to TRACE_PAYLOAD_LEN
// captured bytes per dropped packet, appended to the event ring in batch order
// (per-block counts, an exclusive scan, then a block-local scan for the slots).
struct EvSrc {
    const uint8_t *recs;      // per-packet verdict records
    uint32_t stride, act_off; // record stride, offset of action (reason, ct_ret, flags follow)
    int32_t stage_off;        // pipeline / egress: offset of the stage byte (-1: ingress records)
    const gf_rec *prec;       // handle_policy inputs (src_identity, ifindex, program slot)
    const gf_lxc_dev *cfgs;   // endpoint programs (LXC_ID, SECLABEL)
    const uint32_t *len, *flow_hash;
    const uint8_t *snap;      // frames to capture from (may be null)
    uint32_t snap_stride, n;
    // trace notifications (trace.h:59-106); trace == 0: drop records only
    uint32_t trace, kind;     // kind: 0 ingress, 1 pipeline, 2 egress
    const uint8_t *tmark;     // GF_TR_* per packet
    const uint8_t *tcap_px;   // TO_PROXY captures (GF_TR_CAPTURED)
    const uint8_t *tcap_in;   // pipeline: TRACE_FROM_STACK captures
    const uint8_t *orig;      // egress: the frames as sent (TRACE_FROM_LXC), snap_stride apart
    const uint16_t *lxc_id, *slot_of;   // egress: the sender's program
    uint32_t host_ifindex, encap_ifindex, nd_trace, nd_ifindex;   // nd_trace: 0, or the front program's observation
                                                                  // point | its own final stage << 8
    // from-host (nd_trace's observation point is TR_FROM_HOST): the per-packet choice of
    // TRACE_FROM_HOST / FROM_PROXY is made from the batch's mark column (null: all 0)
    const uint32_t *hmark;
    // debug notifications (dbg.h; ev_list_dbg): the per-packet DbgLog entries of k_ing_groups_dbg
    // (null: none) and the batch's tc_index column (DBG_SKIP_PROXY's argument; may be null)
    const uint4 *dlog;
    const uint8_t *tc_index;
};
// One notification: the 8 header words of struct drop_notify / trace_notify and
// where its captured bytes come from.
struct EvOne {
    uint32_t w[8];
    const uint8_t *pay;       // frame bytes (null: zeros)
    uint32_t pstride;         // bytes present at pay
};
__device__ __forceinline__ EvOne ev_trace(uint32_t obs, uint32_t source, uint32_t hash, uint32_t len, uint32_t src,
                                          uint32_t dst, uint32_t dst_id, uint32_t ifindex, uint32_t reason,
                                          const uint8_t *pay, uint32_t pstride) {
    EvOne e;
    const uint32_t cap = len < GF_TRACE_PAYLOAD_LEN ? len : GF_TRACE_PAYLOAD_LEN;
    e.w[0] = 4u /* CILIUM_NOTIFY_TRACE */ | (obs << 8) | ((source & 0xffffu) << 16);
    e.w[1] = hash; e.w[2] = len; e.w[3] = cap; e.w[4] = src; e.w[5] = dst;
    e.w[6] = (dst_id & 0xffffu) | ((reason & 0xffu) << 16);
    e.w[7] = ifindex;
    e.pay = pay; e.pstride = pstride;
    return e;
}
enum { TR_TO_LXC = 0, TR_TO_PROXY = 1, TR_TO_HOST = 2, TR_TO_STACK = 3, TR_TO_OVERLAY = 4, TR_FROM_LXC = 5,
       TR_FROM_PROXY = 6, TR_FROM_HOST = 7, TR_FROM_STACK = 8, TR_FROM_OVERLAY = 9 };
// The notifications of packet i in the order the programs send them (k < 0:
// just count them).  Drops: send_drop_notify / __send_drop_notify (drop.h:47-107)
// after handle_policy (src_label, SECLABEL, LXC_ID, ifindex), the sender's
// (SECLABEL, 0, 0, 0) after the from-container program, zeros for the callers'
// send_drop_notify_error.  Traces: from_netdev's TRACE_FROM_STACK
// (bpf_netdev.c:436) or from_overlay's TRACE_FROM_OVERLAY (bpf_overlay.c:174), handle_ingress's TRACE_FROM_LXC (bpf_lxc.c:705), the
// redirects' TRACE_TO_PROXY (lxc.h:116/168), TO_HOST / TO_STACK / TO_OVERLAY
// of the from-container exits (bpf_lxc.c:364,381,650,669, encap.h:67) and
// handle_policy's TRACE_TO_LXC when it did not redirect (bpf_lxc.c:1013-1016).
__device__ uint32_t ev_list(const EvSrc &E, uint32_t i, int k, EvOne &out) {
    const uint8_t *r = E.recs + (size_t)i * E.stride;
    const uint32_t act = r[E.act_off], reason = r[E.act_off + 1], ct_ret = r[E.act_off + 2], ofl = r[E.act_off + 3];
    const uint32_t stage = E.stage_off < 0 ? (uint32_t)GF_STAGE_POLICY : r[E.stage_off];
    const uint32_t len = E.len[i], hash = E.flow_hash ? E.flow_hash[i] : 0u;
    const uint8_t *fin = E.snap ? E.snap + (size_t)i * E.snap_stride : nullptr;
    const uint32_t mark = E.tmark ? E.tmark[i] : 0u;
    const uint8_t *pxc = (mark & GF_TR_CAPTURED) ? E.tcap_px + (size_t)i * GF_TRACE_PAYLOAD_LEN : fin;
    const uint32_t pxs = (mark & GF_TR_CAPTURED) ? GF_TRACE_PAYLOAD_LEN : E.snap_stride;
    uint32_t n = 0;
    auto put = [&](const EvOne &e) { if ((int)n == k) out = e; n++; };
    if (E.trace) {
        if (E.kind == 1 && E.nd_trace && (stage == (E.nd_trace >> 8) || stage == GF_STAGE_POLICY)) {
            uint32_t obs = E.nd_trace & 0xffu, src = 0;
            const uint8_t *cin = E.tcap_in + (size_t)i * GF_TRACE_PAYLOAD_LEN;
            // the fronts capture min(snap_stride, 128) bytes of the row: the rest of the slot is not the frame's
            const uint32_t cst = E.snap_stride < GF_TRACE_PAYLOAD_LEN ? E.snap_stride : GF_TRACE_PAYLOAD_LEN;
            if (obs == TR_FROM_HOST) {                      // bpf_netdev.c:423-433: report_identity
                uint32_t skip;
                const uint32_t pid = host_mark_identity(E.hmark ? E.hmark[i] : 0u, skip);
                src = 1u;                                   // HOST_ID
                if (pid) { obs = TR_FROM_PROXY; src = pid; }
                put(ev_trace(obs, 0, hash, len, src, 0, 0, E.nd_ifindex, 0, cin, cst));
                if (stage == GF_STAGE_HOST && act == TC_REDIRECT && !(ofl & GF_PIPE_F_ICMP6_TE)) {
                    // encap_and_redirect's TRACE_TO_OVERLAY (encap.h:67) with the packet's secctx,
                    // which the front left in the record it packed
                    put(ev_trace(TR_TO_OVERLAY, 0, hash, len, E.prec[i].src_identity, 0, 0, E.encap_ifindex, 0, fin,
                                 E.snap_stride));
                }
            } else {
                put(ev_trace(obs, 0, hash, len, 0, 0, 0, E.nd_ifindex, 0, cin, cst));
                if (stage == GF_STAGE_NETDEV && (ofl & GF_PIPE_F_ENCAP))   // GF_NETDEV_F_ENCAP's redirect (encap.h:67), as above
                    put(ev_trace(TR_TO_OVERLAY, 0, hash, len, E.prec[i].src_identity, 0, 0, E.encap_ifindex, 0, fin,
                                 E.snap_stride));
            }
        }
        if (E.kind == 2) {
            const uint32_t sl = E.slot_of[E.lxc_id ? E.lxc_id[i] : 0];
            const gf_lxc_dev *sc = sl ? E.cfgs + (sl - 1) : nullptr;
            if (sc && (gload<uint32_t>(&sc->flags) & GF_LXC_F_TRACE_NOTIFY)) {
                const uint32_t lid = gload<uint32_t>(&sc->lxc_id), sec = gload<uint32_t>(&sc->seclabel);
                const uint32_t fwd = r[5];                 // gf_egress_out.eg_ct_ret
                const uint32_t ef = *reinterpret_cast<const uint16_t *>(r + 14);
                put(ev_trace(TR_FROM_LXC, lid, hash, len, sec, 0, 0, 0, 0, E.orig + (size_t)i * E.snap_stride,
                             E.snap_stride));
                if (mark & GF_TR_PX_EGRESS)
                    put(ev_trace(TR_TO_PROXY, lid, hash, len, sec, 0, 0, E.host_ifindex, fwd, pxc, pxs));
                if (stage == GF_STAGE_FROM_LXC && act != TC_SHOT) {
                    if (ef & GF_EG_F_TO_HOST)
                        put(ev_trace(TR_TO_HOST, lid, hash, len, sec, 1u /* HOST_ID */, 0, E.host_ifindex, fwd, fin,
                                     E.snap_stride));
                    else if (ef & GF_EG_F_TO_STACK)
                        put(ev_trace(TR_TO_STACK, lid, hash, len, sec, (mark & GF_TR_CLUSTER) ? 3u : 2u, 0, 0, fwd, fin,
                                     E.snap_stride));
                    else if (ef & GF_EG_F_ENCAP)
                        put(ev_trace(TR_TO_OVERLAY, lid, hash, len, sec, 0, 0, E.encap_ifindex, 0, fin, E.snap_stride));
                }
            }
        }
        if (stage == GF_STAGE_POLICY) {                    // handle_policy of the destination
            const gf_rec pr = E.prec[i];
            const gf_lxc_dev *dc = pr.ep ? E.cfgs + (pr.ep - 1) : nullptr;
            if (dc && (gload<uint32_t>(&dc->flags) & GF_LXC_F_TRACE_NOTIFY)) {
                const uint32_t lid = gload<uint32_t>(&dc->lxc_id), sec = gload<uint32_t>(&dc->seclabel);
                if (mark & GF_TR_PX_POLICY)
                    put(ev_trace(TR_TO_PROXY, lid, hash, len, sec, 0, 0, E.host_ifindex, ct_ret, pxc, pxs));
                if (act != TC_SHOT && !((ofl & GF_INGRESS_F_PROXY) && pr.ifindex != E.host_ifindex))
                    put(ev_trace(TR_TO_LXC, lid, hash, len, pr.src_identity, sec, lid, pr.ifindex, ct_ret, fin,
                                 E.snap_stride));
            }
        }
    }
    if (act == TC_SHOT && stage != GF_STAGE_XDP && (int)n == k) {
        uint32_t src = 0, dst = 0, dst_id = 0, ifx = 0, source = 0;
        if (stage == GF_STAGE_FROM_LXC) {
            const gf_rec pr = E.prec[i];                // send_drop_notify(skb, SECLABEL, 0, 0, 0, ret) of the sender
            if (pr.ep) { const gf_lxc_dev &cf = E.cfgs[pr.ep - 1]; src = cf.seclabel & 0xffffu; source = cf.lxc_id & 0xffffu; }
        } else if (stage == GF_STAGE_POLICY) {
            const gf_rec pr = E.prec[i];
            if (pr.ep) {                                // handle_policy: send_drop_notify(src_label, SECLABEL, LXC_ID, ifindex)
                const gf_lxc_dev &cf = E.cfgs[pr.ep - 1];
                src = pr.src_identity & 0xffffu; dst = cf.seclabel & 0xffffu;
                dst_id = cf.lxc_id; ifx = pr.ifindex; source = cf.lxc_id & 0xffffu;
            }                                           // else the caller's send_drop_notify_error: zeros
        }
        out.w[0] = 1u /* CILIUM_NOTIFY_DROP */ | (reason << 8) | (source << 16);
        out.w[1] = hash;
        out.w[2] = len; out.w[3] = len < GF_TRACE_PAYLOAD_LEN ? len : GF_TRACE_PAYLOAD_LEN;
        out.w[4] = src; out.w[5] = dst; out.w[6] = dst_id; out.w[7] = ifx;
        out.pay = fin; out.pstride = E.snap_stride;
    }
    if (act == TC_SHOT && stage != GF_STAGE_XDP) n++;
    return n;
}
// Debug notifications (bpf/lib/dbg.h:144-214): struct debug_msg (20 B: type
// CILIUM_NOTIFY_DBG_MSG = 2, subtype, source, hash, arg1..3) and struct
// debug_capture_msg (24 B: type CILIUM_NOTIFY_DBG_CAPTURE = 3, ..., len_orig, len_cap,
// arg1, arg2, then len_cap frame bytes).  In EvOne: the header words first, zeros after.
enum { DBG_GENERIC = 1, DBG_POLICY_DENIED = 5, DBG_CT_MATCH = 8, DBG_CT_VERDICT = 15, DBG_TO_HOST = 19,
       DBG_LB6_REVERSE_NAT_LOOKUP = 26, DBG_LB6_REVERSE_NAT = 27, DBG_LB4_REVERSE_NAT_LOOKUP = 32, DBG_LB4_REVERSE_NAT = 33,
       DBG_REV_PROXY_UPDATE = 40, DBG_L4_POLICY = 41, DBG_CT_LOOKUP4_1 = 44, DBG_CT_LOOKUP4_2 = 45, DBG_CT_CREATED4 = 46,
       DBG_CT_LOOKUP6_1 = 47, DBG_CT_LOOKUP6_2 = 48, DBG_CT_CREATED6 = 49, DBG_SKIP_PROXY = 50, DBG_L4_CREATE = 51,
       DBG_CAPTURE_PROXY_POST = 9 };
__device__ __forceinline__ EvOne ev_dbg(uint32_t sub, uint32_t source, uint32_t hash, uint32_t a1, uint32_t a2,
                                        uint32_t a3 = 0) {
    EvOne e;
    e.w[0] = 2u /* CILIUM_NOTIFY_DBG_MSG */ | (sub << 8) | ((source & 0xffffu) << 16);
    e.w[1] = hash; e.w[2] = a1; e.w[3] = a2; e.w[4] = a3; e.w[5] = e.w[6] = e.w[7] = 0;
    e.pay = nullptr; e.pstride = 0;
    return e;
}
__device__ __forceinline__ EvOne ev_dbg_capture(uint32_t sub, uint32_t source, uint32_t hash, uint32_t len, uint32_t a1,
                                                const uint8_t *pay, uint32_t pstride) {
    EvOne e;
    e.w[0] = 3u /* CILIUM_NOTIFY_DBG_CAPTURE */ | (sub << 8) | ((source & 0xffffu) << 16);
    e.w[1] = hash; e.w[2] = len; e.w[3] = len < GF_TRACE_PAYLOAD_LEN ? len : GF_TRACE_PAYLOAD_LEN;
    e.w[4] = a1; e.w[5] = e.w[6] = e.w[7] = 0;
    e.pay = pay; e.pstride = pstride;
    return e;
}
// The reverse-NAT entry of index idx (raw be16) in the program's map: {nat->address (IPv6:
// address.p4), nat->port} as loaded.  Out of line: the probe loop stays out of the event
// kernels' registers.
__device__ __attribute__((noinline)) uint2 ev_rev_nat_ol(const gf_lxc_dev *dc, bool v6, uint32_t idx) {
    const gf_htab_desc rn = gload<gf_htab_desc>(v6 ? &dc->revnat6 : &dc->revnat4);
    const uint32_t kw[1] = {idx};
    const int64_t f = ht_find<2>(rn, kw, key_hash<2>(kw));
    if (f < 0) return make_uint2(0u, 0u);               // (not reached: the running packet found it)
    const uint8_t *nat = ht_val(rn, f);
    return make_uint2(gload<uint32_t>(nat + (v6 ? 12 : 0)), gload<uint16_t>(nat + (v6 ? 16 : 4)));
}
__device__ __forceinline__ uint32_t ev_ntohs(uint32_t v) { return ((v & 0xffu) << 8) | ((v >> 8) & 0xffu); }
// ev_list for a plain ingress call (kind 0: handle_policy alone) whose array holds a
// program with GF_LXC_F_DEBUG: the cilium_dbg* messages of handle_policy
// (bpf_lxc.c:745-1024 and what it calls) expanded from the packet's DbgLog entry in the
// order they are sent, the program's trace records at their places (TRACE_TO_PROXY
// inside the redirect, lxc.h:116/168; TRACE_TO_LXC last), then the drop record.
// It restates ev_list's kind-0 trace and drop records instead of extending ev_list, and
// ev_write_body keeps ev_list's slot writer next to ev_store, so that k_ev_count /
// k_ev_write stay the code they were: a change of the drop or trace record layout has
// to be made in both places.
__device__ uint32_t ev_list_dbg(const EvSrc &E, uint32_t i, int k, EvOne &out) {
    const uint8_t *r = E.recs + (size_t)i * E.stride;
    const uint32_t act = r[E.act_off], reason = r[E.act_off + 1], ct_ret = r[E.act_off + 2], ofl = r[E.act_off + 3];
    const uint32_t len = E.len[i], hash = E.flow_hash ? E.flow_hash[i] : 0u;
    const uint8_t *fin = E.snap ? E.snap + (size_t)i * E.snap_stride : nullptr;
    const uint32_t mark = E.tmark ? E.tmark[i] : 0u;
    const uint8_t *pxc = (mark & GF_TR_CAPTURED) ? E.tcap_px + (size_t)i * GF_TRACE_PAYLOAD_LEN : fin;
    const uint32_t pxs = (mark & GF_TR_CAPTURED) ? GF_TRACE_PAYLOAD_LEN : E.snap_stride;
    const gf_rec pr = E.prec[i];
    const gf_lxc_dev *dc = pr.ep ? E.cfgs + (pr.ep - 1) : nullptr;
    const uint32_t pfl = dc ? gload<uint32_t>(&dc->flags) : 0u;
    const uint32_t lid = dc ? gload<uint32_t>(&dc->lxc_id) : 0u, sec = dc ? gload<uint32_t>(&dc->seclabel) : 0u;
    const bool tr = E.trace && (pfl & GF_LXC_F_TRACE_NOTIFY);
    uint32_t lw[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (E.dlog && (pfl & GF_LXC_F_DEBUG)) {
        const uint4 a = E.dlog[2 * (size_t)i], b = E.dlog[2 * (size_t)i + 1];
        lw[0] = a.x; lw[1] = a.y; lw[2] = a.z; lw[3] = a.w; lw[4] = b.x; lw[5] = b.y; lw[6] = b.z; lw[7] = b.w;
    }
    const uint32_t bits = lw[0];
    const bool v6 = (pr.cls & 3u) == 2u;
    uint32_t n = 0;
    auto put = [&](const EvOne &e) { if ((int)n == k) out = e; n++; };
    if (bits & GF_DBG_SKIP) put(ev_dbg(DBG_SKIP_PROXY, lid, hash, E.tc_index ? E.tc_index[i] : 1u, 0));
    if (bits & GF_DBG_LOOKUP) {
        // the tuple before the first __ct_lookup (conntrack.h:265-267, 413-415): ct_l4's port word
        uint32_t pw = 0, tfl = 0;
        int action; bool syn;
        (void)ct_l4(pr.proto, v6, pr, pw, tfl, action, syn);
        const uint32_t ports = (ev_ntohs(pw >> 16) << 16) | ev_ntohs(pw & 0xffffu);
        if (v6) put(ev_dbg(DBG_CT_LOOKUP6_1, lid, hash, lw[6], lw[7], ports));
        else put(ev_dbg(DBG_CT_LOOKUP4_1, lid, hash, pr.saddr, pr.daddr, ports));
        put(ev_dbg(v6 ? DBG_CT_LOOKUP6_2 : DBG_CT_LOOKUP4_2, lid, hash, ((uint32_t)pr.proto << 8) | tfl, 0));
        if (bits & GF_DBG_MATCH) put(ev_dbg(DBG_CT_MATCH, lid, hash, lw[1], lw[2]));
        put(ev_dbg(DBG_CT_VERDICT, lid, hash, lw[3], lw[2]));
    }
    // LB_DEBUG (cilium_dbg_lb is cilium_dbg only with both options, lb.h:85-89, dbg.h:134-233):
    // lb{4,6}_rev_nat between ct_lookup and policy_can_access_ingress (bpf_lxc.c:801-808, 909-918).
    // nat->address / nat->port as loaded (be32 / be16; IPv6: address.p4), found again from the
    // logged index in the program's reverse-NAT map, which no kernel writes.
    if ((bits & GF_DBG_REVNAT) && (pfl & GF_LXC_F_LB_DEBUG)) {
        put(ev_dbg(v6 ? DBG_LB6_REVERSE_NAT_LOOKUP : DBG_LB4_REVERSE_NAT_LOOKUP, lid, hash, lw[2], 0));
        if (bits & GF_DBG_REVNAT_HIT) {
            const uint2 nat = ev_rev_nat_ol(dc, v6, lw[2]);
            put(ev_dbg(v6 ? DBG_LB6_REVERSE_NAT : DBG_LB4_REVERSE_NAT, lid, hash, nat.x, nat.y));
        }
    }
    if (bits & GF_DBG_L4_KEY) put(ev_dbg(DBG_L4_CREATE, lid, hash, pr.src_identity, sec, (lw[4] << 16) | pr.proto));
    if (bits & GF_DBG_L4_PROXY) {                       // l4_proxy_lookup (l4.h:191-216)
        put(ev_dbg(DBG_GENERIC, lid, hash, lw[4], pr.proto));
        put(ev_dbg(DBG_L4_POLICY, lid, hash, bits >> 16, 1u /* CT_INGRESS */));
    }
    if (bits & GF_DBG_DENIED) put(ev_dbg(DBG_POLICY_DENIED, lid, hash, pr.src_identity, sec));
    if (bits & GF_DBG_CREATED) {
        if (v6) put(ev_dbg(DBG_CT_CREATED6, lid, hash, lw[7] & 0xffffu, pr.src_identity, 0));
        else put(ev_dbg(DBG_CT_CREATED4, lid, hash, 0, pr.src_identity, 0));
    }
    if (tr && (mark & GF_TR_PX_POLICY))
        put(ev_trace(TR_TO_PROXY, lid, hash, len, sec, 0, 0, E.host_ifindex, ct_ret, pxc, pxs));
    if (bits & GF_DBG_CAPTURE) {                        // ipv{4,6}_redirect_to_host_port (lxc.h:133-136, 184)
        put(ev_dbg_capture(DBG_CAPTURE_PROXY_POST, lid, hash, len, lw[5], fin, E.snap_stride));
        if (!v6) {
            put(ev_dbg(DBG_REV_PROXY_UPDATE, lid, hash, ((pr.l4w0 & 0xffffu) << 16) | lw[5], pr.saddr, pr.proto));
            if (act != TC_SHOT) put(ev_dbg(DBG_TO_HOST, lid, hash, 0, 0));   // (not on DROP_PROXYMAP_CREATE_FAILED)
        }
    }
    if (tr && act != TC_SHOT && !((ofl & GF_INGRESS_F_PROXY) && pr.ifindex != E.host_ifindex))
        put(ev_trace(TR_TO_LXC, lid, hash, len, pr.src_identity, sec, lid, pr.ifindex, ct_ret, fin, E.snap_stride));
    if (act == TC_SHOT) {
        if ((int)n == k) {                              // handle_policy: send_drop_notify(src_label, SECLABEL, LXC_ID, ifindex)
            out.w[0] = 1u /* CILIUM_NOTIFY_DROP */ | (reason << 8) | (dc ? (lid & 0xffffu) << 16 : 0u);
            out.w[1] = hash;
            out.w[2] = len; out.w[3] = len < GF_TRACE_PAYLOAD_LEN ? len : GF_TRACE_PAYLOAD_LEN;
            out.w[4] = dc ? pr.src_identity & 0xffffu : 0u; out.w[5] = dc ? sec & 0xffffu : 0u;
            out.w[6] = dc ? lid : 0u; out.w[7] = dc ? pr.ifindex : 0u;
            out.pay = fin; out.pstride = E.snap_stride;
        }
        n++;
    }
    return n;
}
// One record into its ring slot.  Drop / trace records: 8 header words, the payload
// at byte 32.  DBG: debug_msg has 5 header words and no payload, debug_capture_msg 6
// and its payload at byte 24; the rest of the slot is zero-filled either way.
template <bool DBG>
__device__ __forceinline__ void ev_store(uint32_t *w, const EvOne &e) {
    uint32_t hw = 8, cap = e.w[3];
    if constexpr (DBG) {
        const uint32_t type = e.w[0] & 0xffu;
        if (type == 2u) { hw = 5; cap = 0; } else if (type == 3u) hw = 6;
    }
    for (uint32_t q = 0; q < 8; q++) if (q < hw) w[q] = e.w[q];
    for (uint32_t q = hw; q < GF_EVENT_RECORD / 4; q++) {
        uint32_t v = 0;
        for (uint32_t b = 0; b < 4; b++) {
            const uint32_t off = 4 * (q - hw) + b;
            if (e.pay && off < cap && off < e.pstride) v |= (uint32_t)e.pay[off] << (8 * b);
        }
        w[q] = v;
    }
}
template <bool DBG>
__device__ __forceinline__ uint32_t ev_list_of(const EvSrc &E, uint32_t i, int k, EvOne &out) {
    if constexpr (DBG) return ev_list_dbg(E, i, k, out);
    else return ev_list(E, i, k, out);
}
template <bool DBG>
__device__ __forceinline__ void ev_count_body(const EvSrc &E, uint32_t *blk) {
    __shared__ uint32_t c;
    if (threadIdx.x == 0) c = 0;
    __syncthreads();
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    EvOne e;
    if (i < E.n) { const uint32_t m = ev_list_of<DBG>(E, i, -1, e); if (m) atomicAdd(&c, m); }
    __syncthreads();
    if (threadIdx.x == 0) blk[blockIdx.x] = c;
}
template <bool DBG>
__device__ __forceinline__ void ev_write_body(const EvSrc &E, const uint32_t *boff, const gf_event_ring &R) {
    __shared__ uint32_t sc[BLOCK];
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    EvOne e;
    const uint32_t m = i < E.n ? ev_list_of<DBG>(E, i, -1, e) : 0u;
    sc[threadIdx.x] = m;
    __syncthreads();
    for (uint32_t o = 1; o < BLOCK; o <<= 1) {          // inclusive scan
        uint32_t v = threadIdx.x >= o ? sc[threadIdx.x - o] : 0u;
        __syncthreads();
        sc[threadIdx.x] += v;
        __syncthreads();
    }
    for (uint32_t k = 0; k < m; k++) {
        const uint64_t pos = (uint64_t)*R.count + boff[blockIdx.x] + sc[threadIdx.x] - m + k;
        if (pos >= R.capacity) return;                  // ring full: the record is lost
        ev_list_of<DBG>(E, i, (int)k, e);
        uint32_t *w = reinterpret_cast<uint32_t *>(R.records + pos * GF_EVENT_RECORD);
        if constexpr (DBG) {
            ev_store<true>(w, e);
        } else {
            for (int q = 0; q < 8; q++) w[q] = e.w[q];
            const uint32_t cap = e.w[3];
            for (uint32_t q = 0; q < GF_TRACE_PAYLOAD_LEN / 4; q++) {
                uint32_t v = 0;
                for (uint32_t b = 0; b < 4; b++) {
                    const uint32_t off = 4 * q + b;
                    if (e.pay && off < cap && off < e.pstride) v |= (uint32_t)e.pay[off] << (8 * b);
                }
                w[8 + q] = v;
            }
        }
    }
}
__global__ __launch_bounds__(BLOCK) void k_ev_count(EvSrc E, uint32_t *blk) { ev_count_body<false>(E, blk); }
__global__ __launch_bounds__(BLOCK) void k_ev_write(EvSrc E, const uint32_t *boff, gf_event_ring R) {
    ev_write_body<false>(E, boff, R);
}
// the same two passes over ev_list_dbg (a call whose array holds a program with GF_LXC_F_DEBUG)
__global__ __launch_bounds__(BLOCK) void k_ev_count_dbg(EvSrc E, uint32_t *blk) { ev_count_body<true>(E, blk); }
__global__ __launch_bounds__(BLOCK) void k_ev_write_dbg(EvSrc E, const uint32_t *boff, gf_event_ring R) {
    ev_write_body<true>(E, boff, R);
}
__global__ void k_ev_commit(const uint32_t *boff, const uint32_t *blk, uint32_t nb, gf_event_ring R) {
    *R.count += boff[nb - 1] + blk[nb - 1];
}

// ================================================================ cilium_proxy{4,6} updates
// The redirects of a launch are logged (pol_redirect) and applied here in batch
// order.  The proxy maps change only through these updates while a batch runs,
// so applying them after the launch gives every update the outcome sequential
// execution gives it.  Parallel path (the maps cannot fill): the log is sorted by
// (key hash, packet index); an entry is applied only if no later entry of the
// batch has the same key (the last writer wins, as in order), and distinct keys
// insert concurrently.  Sequential path (a map could fill): one lane applies the
// log in packet order with exact max_entries accounting; a failed update turns
// the packet into DROP_PROXYMAP_CREATE_FAILED (lxc.h:137/199).  Successful
// redirects get ipv{4,6}_policy's MAC stores (bpf_lxc.c:840-846, 955-961).
struct PxDev {
    gf_htab_desc d4, d6;
    uint8_t *snap;              // writable frames (pipeline) or null
    const uint32_t *len;
    uint32_t snap_stride;
    uint32_t host_mac[2], node_mac[2];
};
__device__ __forceinline__ bool px_same(const uint32_t *a, const uint32_t *b) {
    if (a[1] != b[1]) return false;
    const int nw = a[1] == 6 ? 6 : 3;
    for (int k = 0; k < nw; k++) if (a[2 + k] != b[2 + k]) return false;
    return true;
}
__device__ __forceinline__ void px_macs(const PxDev &P, uint32_t i) {
    if (!P.snap) return;
    const uint32_t len = P.len[i];
    Row w{P.snap + (size_t)i * P.snap_stride, P.snap_stride < len ? P.snap_stride : len};
    w.w32(6, P.node_mac[0]); w.w16(10, P.node_mac[1]);     // eth_store_saddr(NODE_MAC)
    w.w32(0, P.host_mac[0]); w.w16(4, P.host_mac[1]);      // eth_store_daddr(HOST_IFINDEX_MAC)
}
__device__ __forceinline__ int64_t px_upsert(const PxDev &P, const uint32_t *e, bool strict, int *added) {
    if (e[1] == 6) return P.d6.slots ? ht_upsert<22, 7, GF_HASH_PLAIN>(P.d6, e + 2, e + 8, strict, added) : 0;
    return P.d4.slots ? ht_upsert<10, 4, GF_HASH_PLAIN>(P.d4, e + 2, e + 8, strict, added) : 0;
}
// Without proxy maps the updates are no-ops: only the redirects' MAC stores (frames written)
__global__ __launch_bounds__(BLOCK) void k_px_macs(const uint32_t *plog, const uint32_t *n_, PxDev P) {
    const uint32_t n = *n_;
    for (uint32_t j = blockIdx.x * BLOCK + threadIdx.x; j < n; j += gridDim.x * BLOCK) {
        const uint32_t *e = plog + 16ull * j;
        if (!e[15]) px_macs(P, e[0]);
    }
}
__global__ __launch_bounds__(BLOCK) void k_px_keys(const uint32_t *plog, uint32_t n, bool by_index,
                                                   unsigned long long *key, uint32_t *val) {
    const uint32_t j = blockIdx.x * BLOCK + threadIdx.x;
    if (j >= n) return;
    const uint32_t *e = plog + 16ull * j;
    uint32_t h = 0;
    if (!by_index) h = e[1] == 6 ? key_hash<22>(e + 2) : key_hash<10>(e + 2);
    key[j] = ((unsigned long long)h << 32) | e[0];
    val[j] = j;
}
__global__ __launch_bounds__(BLOCK) void k_px_apply(const uint32_t *plog, uint32_t n, const unsigned long long *key,
                                                    const uint32_t *perm, PxDev P) {
    const uint32_t p = blockIdx.x * BLOCK + threadIdx.x;
    if (p >= n) return;
    const uint32_t *e = plog + 16ull * perm[p];
    if (!e[15]) px_macs(P, e[0]);
    const uint32_t h = (uint32_t)(key[p] >> 32);
    for (uint32_t q = p + 1; q < n && (uint32_t)(key[q] >> 32) == h; q++)
        if (px_same(e, plog + 16ull * perm[q])) return;     // a later update of the same key wins
    int added = 0;
    px_upsert(P, e, false, &added);
    if (added) atomicAdd(e[1] == 6 ? P.d6.count : P.d4.count, (uint32_t)added);
}
__global__ void k_px_apply_seq(const uint32_t *plog, uint32_t n, const uint32_t *perm, PxDev P, uint8_t *recs,
                               uint32_t stride, uint32_t act_off, unsigned long long *stats) {
    for (uint32_t p = 0; p < n; p++) {
        const uint32_t *e = plog + 16ull * perm[p];
        const uint32_t i = e[0];
        if (px_upsert(P, e, true, nullptr) >= 0) { if (!e[15]) px_macs(P, i); continue; }
        uint8_t *r = recs + (size_t)i * stride;             // DROP_PROXYMAP_CREATE_FAILED
        const uint32_t old_action = r[act_off];
        r[act_off] = TC_SHOT; r[act_off + 1] = 161;
        if (stride == 8) { r[3] &= 2; r[4] = r[5] = r[6] = r[7] = 0; }
        else { r[4] &= ~1u; r[6] = r[7] = r[8] = r[9] = 0; }
        if (stats) {
            atomicAdd(&stats[0], ~0ull); atomicAdd(&stats[161], 1ull);
            atomicAdd(&stats[256 + old_action], ~0ull); atomicAdd(&stats[256 + TC_SHOT], 1ull);
        }
    }
}

// ================================================================ endpoint egress (from-container)
// handle_ingress (bpf/bpf_lxc.c:685-738) -> tail_handle_ipv4 -> handle_ipv4_from_lxc
// (:427-658) over frames sent by local endpoints.  k_eg_front runs the stateless
// part on one packet per lane (checks, lb4_local with its lb4_xlate rewrites,
// map_lxc_out) and keys the packet by the flow group of its CT tuple; the
// schedule of the ingress path orders the groups; k_eg_groups runs the CT /
// policy part of each bucket on one lane in batch order, ending in a verdict or
// in ipv4_local_delivery, whose handle_policy runs in the ingress pass after it.
// ct_create4's service entry (conntrack.h:533-561) has the pair {target, target}
// or {IPV4_LOOPBACK, sender}, outside the packet's group: it is logged and
// applied after the launch in batch order (last writer wins, as in order).  No
// packet of the batch reads such a key unless its own tuple has that shape
// (saddr == daddr, or IPV4_LOOPBACK in it); k_eg_front flags those batches and
// they run as a single bucket with the entry written inline.
enum {
    D_INVALID_SMAC = -130, D_INVALID_DMAC = -131, D_INVALID_SIP = -132, D_NO_LXC = -152, D_CSUM_L3 = -153,
    D_POLICY_CIDR = -162,
};
#define GF_EGR_FINAL 1u                 // EgRec.st: the verdict was written by k_eg_front
struct __attribute__((aligned(16))) EgRec {   // 32 B: what the CT part needs from the front
    uint32_t t_daddr, t_saddr;          // CT tuple addresses after lb4_local
    uint32_t len, orig_dip;             // skb->len; orig_dip (tuple.daddr after lb4_local)
    uint32_t ct_addr;                   // ct_state_new.addr (0: not load balanced)
    uint16_t rev_nat, ep;               // ct_state_new.rev_nat_index; program slot + 1
    int16_t  l4_off;
    uint8_t  nh, st;
    uint16_t slave, eflags;             // lb4_local's slave; GF_EG_F_* so far
};
static_assert(sizeof(EgRec) == 32, "EgRec must be 32 bytes");
struct EgDev {
    const gf_lxc_dev *cfgs;
    uint8_t *v6blk;                     // per front block: holds an IPv6 frame (k_eg_front<4> writes, <6> reads), or null
    const uint16_t *slot_of;
    gf_key_cfg K;                       // the call's bucket key (gf_key_for(n))
    gf_htab_desc ct4, ct6, lxc, tunnel;
    const uint32_t *lxset, *tnset;      // cilium_lxc's / the tunnel map's IPv4 keys: address set + slots
    uint32_t lxbits, lxzero, tnbits, tnzero;   // (Map::addr_set), or null
    uint8_t *snap;                      // the frames, rewritten in place
    uint8_t *s6out, *d6out;             // IPv6 addresses of the local deliveries (handle_policy's columns)
    uint32_t stride, now, host_ifindex, encap_ifindex;
    uint32_t cluster_range, cluster_mask, loopback, ipv4_mask;
    uint32_t host_mac[2];
    uint32_t router6[4], host6[4];      // ROUTER_IP, HOST_IP (LE words)
    uint32_t strict;                    // bit0: CT4 inserts check max_entries (forces the single bucket); bit1: CT6
    uint32_t *seq;                      // device word: 1 = single-bucket batch (written by k_eg_front)
    uint32_t *ctlog, *ctlog_n;          // deferred service entries {i, key[4], value[12], pad[3]}; [n, v6 deliveries]
    IngCtx X;                           // redirect writes + cilium_proxy4 log (pol_redirect)
    uint64_t *hz_k;                     // per packet, GF_HZ_NK keys (hz_key order below), n apart
    const uint32_t *vip4;               // the rev-NAT addresses of the programs' revNAT maps (open addressing,
    const uint4 *vip6;                  //   0 = empty), vip*_mask + 1 slots; null: none
    uint32_t vip4_mask, vip6_mask;
    uint8_t *hz_fl;                     // per packet: GF_HZ_* (null: no ordering check)
    uint32_t *hz;                       // device words: [0] 1 = ordering hazard (k_eg_groups idles), [1] GF_HZ_* kinds seen
    // Connection groups (IPv4): conn = 1 keys IPv4 packets by their
    // connection and logs the ICMP-related entries ct_create4 writes (the only CT key
    // two connections of a pair share, read only by ICMP errors); an IPv4 ICMP packet
    // in the run sets *cflag and the run falls back to address-pair groups.
    uint32_t conn;
    uint32_t *cflag;                    // device word: 1 = pair groups (an IPv4 ICMP packet reaches conntrack)
    uint32_t *keysP, *key2P;            // the pair keys of the front / of the deliveries (fallback)
    uint32_t *rlog, *rlog_n;            // logged related entries {order, key[4], value[12], pad[3]}
    RelSet rs;                          // their set instead (slot null: the log)
    gf_rec *rec2;                       // the handle_policy pass's records: the front writes every packet's
    uint32_t *key2;                     //   as "not delivered" in batch order, k_eg_groups only the deliveries
};
// The ordering check.  The reference runs a local delivery's
// handle_policy right after its from-container program, before the next packet;
// the batch runs every from-container part first, then every handle_policy.  The
// two orders differ only when a packet's from-container part touches a CT entry an
// earlier packet's handle_policy touches.  The CT keys a packet can touch follow
// from its tuples (conntrack.h:170-289 lookups, :446-580 creates):
//  * handle_policy: its tuple (the frame after the from-container rewrites) and
//    the reverse, for ICMP the related entry of the address pair;
//  * from-container: its CT tuple (after lb4_local) and the reverse, the related
//    entry of the pair for ICMP, and lb4_local's loopback service entry (the frame
//    pair after the SNAT).
// A handle_policy tuple and a later from-container tuple share an entry only in
// opposite directions (the lookups differ in TUPLE_F_IN); so the front keys each
// packet by the connection of its frame tuple and of its CT tuple (unordered 5-tuple,
// ICMP ports 0, + direction), their address pairs, and its two addresses:
//   a later packet whose CT connection equals an earlier frame connection in the
//     other direction (a reply in the same batch);
//   an ICMP packet after any packet of its CT pair, any packet after an ICMP packet
//     of its pair (the related entries);
//   a loopback packet whose frame connection appeared earlier (its service entry);
//   a packet to a rev-NAT address without translation after any packet with its
//     source address (a reply rev-NATed by lb4/6_rev_nat reaches handle_policy as
//     {service address, one of its own addresses});
// flags the batch, which then runs in contiguous runs free of these, in order.
#define GF_HZ_NK      6u                // keys per packet: conn(frame), conn(CT), pair(frame), pair(CT), src, dst
#define GF_HZ_VALID   1u                // continues past the front
#define GF_HZ_DIRI    2u                // direction of the frame tuple within its connection
#define GF_HZ_DIRE    4u                // direction of the CT tuple within its connection
#define GF_HZ_ICMP    8u                // ICMP / ICMPv6
#define GF_HZ_VIP    16u                // to a rev-NAT address without lb4/6_local translation
#define GF_HZ_LOOP   32u                // lb4_local back to the sender (loopback SNAT)
#define GF_HZ_V6     64u                // the IPv6 path
#define GF_HZ_DLV   128u                // may reach ipv4/6_local_delivery (daddr an endpoint, or IPV4_LOOPBACK
                                        // whose rev-NAT restores the sender): only these enter handle_policy
// A CT map that could fill during the batch (strict accounting) makes every
// insert order-dependent (E2BIG for whichever comes last): a batch with a
// continuing packet of that family is flagged 2 and runs one packet at a time.
#define GF_HZ_ICMPSALT 0x6a09e667f3bcc908ull   // the related-entry space of ICMP packets' pairs
#define GF_CTLOG_WORDS 20u

// The header bytes the IPv4 egress programs touch (< l4_off + 18 <= 92) are staged
// per lane in LDS: one vector load per row instead of a global access per byte.
#define GF_EG_STAGE 128u
GF_HD uint32_t eg_stage_bytes(uint32_t S) { return S < GF_EG_STAGE ? S : GF_EG_STAGE; }
// k_eg_groups' LDS row: sized by the snap stride
GF_HD uint32_t eg_row_bytes(uint32_t S) { return (eg_stage_bytes(S) + 15u) & ~15u; }
__device__ __forceinline__ void eg_copy(uint8_t *dst, const uint8_t *src, uint32_t n) {
    if (!(n & 15u) && !(((uintptr_t)src | (uintptr_t)dst) & 15u)) {
        for (uint32_t k = 0; k < n; k += 16) *reinterpret_cast<uint4 *>(dst + k) = *reinterpret_cast<const uint4 *>(src + k);
    } else {
        for (uint32_t k = 0; k < n; k++) dst[k] = src[k];
    }
}
__device__ __forceinline__ bool mac_eq(const Row &w, uint32_t off, const uint32_t *m) {
    return w.r32(off) == m[0] && w.r16(off + 4) == (m[1] & 0xffffu);
}
// ipv4_l3 (bpf/lib/l3.h:54-70) + ipv4_dec_ttl (bpf/lib/ipv4.h:30-43); smac may be null
__device__ __forceinline__ int eg_ipv4_l3(Row &w, uint32_t len, const uint32_t *smac, const uint32_t *dmac) {
    const uint32_t ttl = w.b(22);
    if (ttl <= 1) return D_INVALID;
    l3_csum(w, len, 24, ttl, ttl - 1, 2);
    w.w8(22, ttl - 1);
    if (smac) { w.w32(6, smac[0]); w.w16(10, smac[1] & 0xffffu); }
    w.w32(0, dmac[0]); w.w16(4, dmac[1] & 0xffffu);
    return TC_OK;
}

// handle_ipv6 (bpf_lxc.c:388-416) + the stateless head of ipv6_l3_from_lxc (:120-185):
// icmp6_handle's responders, the source checks, ipv6_hdrlen, lb6_extract_key +
// lb6_lookup_service + lb6_local (lb6_xlate: daddr, the L4 checksum at l4_off + its
// offset even when that offset is 0, the port), map_lxc_out.  TC_OK: continue in
// k_eg_groups (r.st = 0); a stage-NONE responder returns TC_OK with r.st set.
__device__ __forceinline__ int eg_front6(const EgDev &E, const gf_lxc_dev *c, Row &w, uint32_t len, uint32_t fh,
                                         EgRec &r, gf_egress_out &o, uint32_t &ab) {
    r.eflags = GF_EG_F_IPV6;
    if (len < 54) return D_INVALID;
    if (w.b(20) == 58) {                                // icmp6_handle (bpf/lib/icmp6.h:380-401)
        if (len < 62) return D_INVALID;
        const uint32_t type = w.b(54);
        bool to_router = true;
        for (int k = 0; k < 4; k++) to_router &= w.r32(38 + 4 * k) == E.router6[k];
        if (type == 135 || (type == 128 && to_router)) {
            o.stage = GF_STAGE_NONE; o.eg_flags = GF_EG_F_IPV6 | GF_EG_F_RESPONDER;
            return TC_OK;
        }
    }
    uint32_t m[2];
    m[0] = gload<uint32_t>(&c->lxc_mac[0]); m[1] = gload<uint32_t>(&c->lxc_mac[1]);
    if (!mac_eq(w, 6, m)) return D_INVALID_SMAC;
    m[0] = gload<uint32_t>(&c->node_mac[0]); m[1] = gload<uint32_t>(&c->node_mac[1]);
    if (!mac_eq(w, 0, m)) return D_INVALID_DMAC;
    for (int k = 0; k < 4; k++)
        if (w.r32(22 + 4 * k) != gload<uint32_t>(&c->lxc_ip6[k])) return D_INVALID_SIP;
    PktHdr h;
    parse_row(w.p, w.cap, len, h);                      // nexthdr / l4_off after ipv6_hdrlen (negative: added as is)
    const uint32_t nh = h.proto;
    const int l4_off = h.l4;
    r.nh = (uint8_t)nh; r.l4_off = (int16_t)l4_off;
    ab += 34 + 28;
    const uint32_t co = csum_l4_offset(nh), fl = nh == 17 ? GF_F_MANGLED_0 : 0u;
    bool lb_try = true;
    uint32_t kport = 0;
    if (nh == 6 || nh == 17) {
        if (!skb_ok(l4_off + 2, 2, len)) return -GF_EFAULT;
        kport = w.r16((uint32_t)(l4_off + 2));
    } else if (nh != 1 && nh != 58) lb_try = false;
    const gf_htab_desc lb = gload<gf_htab_desc>(&c->lb6);
    if (lb_try && lb.slots) {
        const uint8_t *svc = nullptr;
        if (kport) {
            uint32_t kw[5] = {h.d6[0], h.d6[1], h.d6[2], h.d6[3], kport};
            const int64_t f = ht_find<20>(lb, kw, key_hash<20>(kw));
            ab += 44;
            if (f >= 0) { const uint8_t *v = ht_val(lb, f); if (gload<uint16_t>(v + 18)) svc = v; }
            if (!svc) kport = 0;
        }
        if (!svc) {
            uint32_t kw[5] = {h.d6[0], h.d6[1], h.d6[2], h.d6[3], kport};
            const int64_t f = ht_find<20>(lb, kw, key_hash<20>(kw));
            ab += 44;
            if (f >= 0) { const uint8_t *v = ht_val(lb, f); if (gload<uint16_t>(v + 18)) svc = v; }
        }
        if (svc) {                                      // lb6_local, lb.h:425-445
            const uint32_t count = gload<uint16_t>(svc + 18);
            const uint32_t slave = (fh % count + 1u) & 0xffffu;
            uint32_t kw[5] = {h.d6[0], h.d6[1], h.d6[2], h.d6[3], kport | (slave << 16)};
            const int64_t f = ht_find<20>(lb, kw, key_hash<20>(kw));
            ab += 44;
            if (f < 0) return D_NO_SERVICE;
            const uint8_t *be = ht_val(lb, f);
            r.slave = (uint16_t)slave; r.eflags |= GF_EG_F_LB;
            r.rev_nat = gload<uint16_t>(be + 20);
            uint32_t sum = 0;
            for (int k = 0; k < 4; k++) {               // lb6_xlate: ipv6_store_daddr + csum_diff
                const uint32_t nw = gload<uint32_t>(be + 4 * k);
                w.w32(38 + 4 * k, nw);
                sum = ck_add(ck_add(sum, ~h.d6[k]), nw);
            }
            if (l4_csum(w, len, l4_off + (int)co, 0, sum, GF_F_PSEUDO_HDR | fl) < 0) return D_CSUM_L4;
            const uint32_t sp = gload<uint16_t>(be + 16);
            if (sp && kport != sp && (nh == 6 || nh == 17)) {
                if (l4_csum(w, len, l4_off + (int)co, kport, sp, 2u | fl) < 0) return D_CSUM_L4;
                if (!skb_ok(l4_off + 2, 2, len)) return D_WRITE_ERROR;
                w.w16((uint32_t)(l4_off + 2), sp);
            }
            ab += 24;
        }
    }
    const uint32_t npm = gload<uint32_t>(&c->n_portmap);          // map_lxc_out
    if (npm && (nh == 6 || nh == 17)) {
        if (!skb_ok(l4_off, 2, len)) return D_INVALID;
        const uint32_t sp = w.r16((uint32_t)l4_off);
        for (uint32_t k = 0; k < npm && k < 16; k++) {
            const uint32_t pm = gload<uint32_t>(&c->portmap[k]);
            const uint32_t from = pm & 0xffffu, to = pm >> 16;
            if (to != sp) continue;
            if (l4_csum(w, len, l4_off + (int)co, sp, from, 2u | fl) < 0) return D_CSUM_L4;
            if (!skb_ok(l4_off, 2, len)) return D_WRITE_ERROR;
            w.w16((uint32_t)l4_off, from);
            r.eflags |= GF_EG_F_PORTMAP;
        }
    }
    r.st = 0;
    return TC_OK;
}

// handle_ingress + the stateless head of handle_ipv4_from_lxc, one packet per lane
// FAM 6 takes the IPv6 frames, FAM 4 every other frame (two launches: the IPv6
// path's registers and stack stay out of the IPv4 kernel).
// the slot of a rev-NAT address (fmix32: raw be32 addresses share their low bytes)
GF_HD uint32_t vip_slot(uint32_t x) {
    x ^= x >> 16; x *= 0x85ebca6bu; x ^= x >> 13; x *= 0xc2b2ae35u; x ^= x >> 16;
    return x;
}
__device__ __forceinline__ bool vip4_has(const EgDev &E, uint32_t a) {
    if (!E.vip4 || !a) return false;
    uint32_t slot = vip_slot(a) & E.vip4_mask;
    for (uint32_t k = 0; k <= E.vip4_mask; k++) {
        const uint32_t v = E.vip4[slot];
        if (v == a) return true;
        if (!v) return false;
        slot = (slot + 1u) & E.vip4_mask;
    }
    return false;
}
__device__ __forceinline__ bool vip6_has(const EgDev &E, const uint32_t *a) {
    if (!E.vip6 || !(a[0] | a[1] | a[2] | a[3])) return false;
    uint32_t slot = vip_slot(a[0] ^ vip_slot(a[1] ^ vip_slot(a[2] ^ vip_slot(a[3])))) & E.vip6_mask;
    for (uint32_t k = 0; k <= E.vip6_mask; k++) {
        const uint4 v = E.vip6[slot];
        if (v.x == a[0] && v.y == a[1] && v.z == a[2] && v.w == a[3]) return true;
        if (!(v.x | v.y | v.z | v.w)) return false;
        slot = (slot + 1u) & E.vip6_mask;
    }
    return false;
}
__device__ __forceinline__ uint64_t hz_mix(uint64_t h, uint64_t v) {
    h ^= v + 0x9e3779b97f4a7c15ull + (h << 6) + (h >> 2);
    h *= 0xff51afd7ed558ccdull;
    return h ^ (h >> 31);
}
// Connection key of a tuple: order-free hash of {(sa, sp), (da, dp)} + nexthdr;
// dir = the (sa, sp) side sorts second.
__device__ __forceinline__ uint64_t hz_key(const uint32_t *sa, const uint32_t *da, int nw, uint32_t sp, uint32_t dp,
                                           uint32_t nh, bool &dir) {
    int c = 0;
    for (int k = 0; k < nw && !c; k++) c = sa[k] < da[k] ? -1 : (sa[k] > da[k] ? 1 : 0);
    if (!c) c = sp < dp ? -1 : (sp > dp ? 1 : 0);
    dir = c > 0;
    const uint32_t *lo = dir ? da : sa, *hi = dir ? sa : da;
    uint64_t h = 0x5eed0000ull | (uint64_t)nw;
    for (int k = 0; k < nw; k++) h = hz_mix(h, lo[k]);
    h = hz_mix(h, dir ? dp : sp);
    for (int k = 0; k < nw; k++) h = hz_mix(h, hi[k]);
    h = hz_mix(h, ((dir ? sp : dp) << 8) | nh);
    return h | 1ull;
}

template <int FAM>
__global__ __launch_bounds__(BLOCK) void k_eg_front(gf_frames fr, const uint16_t *lxc_id, const uint32_t *fhash, EgDev E,
                                                    EgRec *erec, uint32_t *keys, gf_egress_out *out,
                                                    unsigned long long *stats) {
    if (FAM == 6 && E.v6blk && !E.v6blk[blockIdx.x]) return;   // no IPv6 frame in this block
    __shared__ uint32_t sl[272];
    extern __shared__ uint4 lds[];                      // BLOCK * eg_stage_bytes(S) (FAM 6: none)
    Stats st{sl};
    if (stats) st.init();
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    const uint32_t S = fr.snap_stride;
    const uint32_t len = i < fr.n ? fr.len[i] : 0u;
    const uint8_t *src = fr.snap + (size_t)i * S;
    const uint32_t cap0 = S < len ? S : len;
    // IPv4 frames that fit a row (and 16-B aligned): the block stages its frames
    // with coalesced 16-B loads and stores them back the same way at the end
    // (block-uniform); otherwise each lane stages its own header.
    const bool coop = FAM == 4 && S <= GF_EG_STAGE && !(S & 15u) &&
                      !(((uintptr_t)fr.snap | (uintptr_t)E.snap) & 15u);
    const uint32_t b0 = blockIdx.x * BLOCK;
    const uint32_t nv = b0 < fr.n ? ((fr.n - b0 < BLOCK ? fr.n - b0 : BLOCK) * S) / 16 : 0u;
    if (coop) {
        const uint4 *g = reinterpret_cast<const uint4 *>(fr.snap + (size_t)b0 * S);
        for (uint32_t k = threadIdx.x; k < nv; k += BLOCK) lds[k] = g[k];
        __syncthreads();
    }
    uint8_t *row = reinterpret_cast<uint8_t *>(lds) + (FAM == 6 ? 0 : threadIdx.x * (coop ? S : eg_stage_bytes(S)));
    const uint8_t *hdr = coop ? row : src;
    const bool v6 = i < fr.n && len >= 14 && fbyte(hdr, cap0, 12) == 0x86 && fbyte(hdr, cap0, 13) == 0xDD;
    if (FAM == 4 && E.v6blk) {                                // tells k_eg_front<6> which blocks to run
        const int any6 = __syncthreads_or(v6 ? 1 : 0);
        if (threadIdx.x == 0) E.v6blk[blockIdx.x] = any6 ? 1u : 0u;
    }
    bool scnt = false;                                        // the lane's counter-block entry
    uint32_t sreason = 0, saction = 0, slen = 0, sab = 0;
    if (i < fr.n && v6 == (FAM == 6)) {
        const uint32_t K = eg_stage_bytes(S);
        uint8_t *dst = E.snap + (size_t)i * S;
        if (FAM == 6) {                                       // extension headers: the whole snap, in HBM
            if (src != dst) eg_copy(dst, src, S);
        } else if (!coop) {
            eg_copy(row, src, K);                             // the header, staged
            if (S > K && src != dst) eg_copy(dst + K, src + K, S - K);   // the rest of the snap, as is
        }
        Row w{row, K < len ? K : len};                        // IPv4: the LDS copy (ds_* accesses)
        Row wg{dst, cap0};                                    // IPv6: the frame in HBM
        gf_egress_out o{};
        EgRec r{};
        r.len = len;
        uint32_t ab = 24 + 34;                            // output record, header bytes parsed
        const uint32_t sl_ = E.slot_of[lxc_id ? lxc_id[i] : 0];
        r.ep = (uint16_t)sl_;
        r.st = GF_EGR_FINAL;
        int ret = TC_OK;
        o.stage = GF_STAGE_FROM_LXC;
        const uint32_t et = len >= 14 ? ((fbyte(src, cap0, 12) << 8) | fbyte(src, cap0, 13)) : 0u;
        do {
            if (!sl_) { ret = D_MISSED_TAIL_CALL; break; }
            const gf_lxc_dev *c = E.cfgs + (sl_ - 1);
            const uint32_t flags = gload<uint32_t>(&c->flags);
            if (et == 0x0806) { o.stage = GF_STAGE_NONE; o.eg_flags = GF_EG_F_ARP; break; }
            if (flags & GF_LXC_F_DROP_ALL) { ret = D_POLICY; break; }
            if constexpr (FAM == 6) { ret = eg_front6(E, c, wg, len, fhash ? fhash[i] : 0u, r, o, ab); break; }
            if (et != 0x0800) { ret = D_UNKNOWN_L3; break; }
            if (len < 34) { ret = D_INVALID; break; }
            const uint32_t nh = w.b(23);
            uint32_t m[2];
            m[0] = gload<uint32_t>(&c->lxc_mac[0]); m[1] = gload<uint32_t>(&c->lxc_mac[1]);
            if (!mac_eq(w, 6, m)) { ret = D_INVALID_SMAC; break; }
            m[0] = gload<uint32_t>(&c->node_mac[0]); m[1] = gload<uint32_t>(&c->node_mac[1]);
            if (!mac_eq(w, 0, m)) { ret = D_INVALID_DMAC; break; }
            const uint32_t saddr = w.r32(26), daddr = w.r32(30);
            if (!(flags & GF_LXC_F_LXC_IPV4) || saddr != gload<uint32_t>(&c->lxc_ipv4)) { ret = D_INVALID_SIP; break; }
            const int l4_off = 14 + (int)(w.b(14) & 0xfu) * 4;
            const uint32_t co = csum_l4_offset(nh), fl = nh == 17 ? GF_F_MANGLED_0 : 0u;
            r.t_daddr = daddr; r.t_saddr = saddr; r.nh = (uint8_t)nh; r.l4_off = (int16_t)l4_off;
            // lb4_extract_key (CT_EGRESS: key.address = daddr) + extract_l4_port (lb.h:191-215, 552-564)
            bool lb_try = true;
            uint32_t kport = 0;
            if (nh == 6 || nh == 17) {
                if (!skb_ok(l4_off + 2, 2, len)) { ret = -GF_EFAULT; break; }
                kport = w.r16((uint32_t)(l4_off + 2));
            } else if (nh != 1 && nh != 58) lb_try = false;     // DROP_UNKNOWN_L4: skip_service_lookup
            const gf_htab_desc lb = gload<gf_htab_desc>(&c->lb4);
            if (lb_try && lb.slots) {
                // lb4_lookup_service (lb.h:566-597), LB_L4 then LB_L3
                const uint8_t *svc = nullptr;
                ab += 12;
                if (kport) {
                    uint32_t kw[2] = {daddr, kport};
                    const int64_t f = ht_find<8>(lb, kw, key_hash<8>(kw));
                    ab += 20;
                    if (f >= 0) { const uint8_t *v = ht_val(lb, f); if (gload<uint16_t>(v + 6)) svc = v; }
                    if (!svc) kport = 0;
                }
                if (!svc) {
                    uint32_t kw[2] = {daddr, kport};
                    const int64_t f = ht_find<8>(lb, kw, key_hash<8>(kw));
                    ab += 20;
                    if (f >= 0) { const uint8_t *v = ht_val(lb, f); if (gload<uint16_t>(v + 6)) svc = v; }
                }
                if (svc) {                                    // lb4_local, lb.h:662-699
                    const uint32_t count = gload<uint16_t>(svc + 6);
                    const uint32_t slave = ((fhash ? fhash[i] : 0u) % count + 1u) & 0xffffu;
                    uint32_t kw[2] = {daddr, kport | (slave << 16)};
                    const int64_t f = ht_find<8>(lb, kw, key_hash<8>(kw));
                    ab += 20;
                    if (f < 0) { ret = D_NO_SERVICE; break; }
                    const uint8_t *be = ht_val(lb, f);
                    const uint32_t target = gload<uint32_t>(be), sport_ = gload<uint16_t>(be + 4);
                    r.slave = (uint16_t)slave; r.eflags |= GF_EG_F_LB;
                    r.rev_nat = gload<uint16_t>(be + 8);
                    r.ct_addr = target;
                    uint32_t new_saddr = 0;
                    if (saddr == target) {                    // loopback back to the sender
                        new_saddr = E.loopback; r.ct_addr = new_saddr; r.eflags |= GF_EG_F_LOOPBACK;
                    } else r.t_daddr = target;
                    // lb4_xlate (lb.h:615-659)
                    w.w32(30, target);
                    uint32_t sum = ck_add(ck_add(0u, ~daddr), target);
                    if (new_saddr) {
                        w.w32(26, new_saddr);
                        sum = ck_add(sum, ck_add(ck_add(0u, ~saddr), new_saddr));
                    }
                    l3_csum(w, len, 24, 0, sum, 0);
                    if (co && l4_csum(w, len, l4_off + (int)co, 0, sum, GF_F_PSEUDO_HDR | fl) < 0) { ret = D_CSUM_L4; break; }
                    if (sport_ && kport != sport_ && (nh == 6 || nh == 17)) {   // l4_modify_port
                        if (l4_csum(w, len, l4_off + (int)co, kport, sport_, 2u | fl) < 0) { ret = D_CSUM_L4; break; }
                        if (!skb_ok(l4_off + 2, 2, len)) { ret = D_WRITE_ERROR; break; }
                        w.w16((uint32_t)(l4_off + 2), sport_);
                    }
                    ab += 12;
                }
            }
            r.orig_dip = r.t_daddr;
            // map_lxc_out (bpf_lxc.c:80-108) + l4_port_map_out (l4.h:107-118)
            const uint32_t npm = gload<uint32_t>(&c->n_portmap);
            if (npm && (nh == 6 || nh == 17)) {
                if (!skb_ok(l4_off, 2, len)) { ret = D_INVALID; break; }
                const uint32_t sp = w.r16((uint32_t)l4_off);
                bool bad = false;
                for (uint32_t k = 0; k < npm && k < 16; k++) {
                    const uint32_t pm = gload<uint32_t>(&c->portmap[k]);
                    const uint32_t from = pm & 0xffffu, to = pm >> 16;
                    if (to != sp) continue;
                    if (l4_csum(w, len, l4_off + (int)co, sp, from, 2u | fl) < 0) { ret = D_CSUM_L4; bad = true; break; }
                    if (!skb_ok(l4_off, 2, len)) { ret = D_WRITE_ERROR; bad = true; break; }
                    w.w16((uint32_t)l4_off, from);
                    r.eflags |= GF_EG_F_PORTMAP;
                }
                if (bad) break;
            }
            r.st = 0;                                       // continue in k_eg_groups
        } while (0);
        uint32_t key;
        if (E.hz_fl) {
            uint64_t K[GF_HZ_NK] = {0, 0, 0, 0, 0, 0};
            uint32_t hfl = 0;
            if (r.st == 0) {
                const int lo4 = r.l4_off;
                const bool tu = (r.nh == 6 || r.nh == 17) && skb_ok(lo4 + 0, 4, len);
                bool di = false, de = false, pd;
                if (FAM == 6) {
                    const uint32_t sp = tu ? wg.r16((uint32_t)lo4) : 0u, dp = tu ? wg.r16((uint32_t)lo4 + 2u) : 0u;
                    uint32_t s6[4], d6[4];
                    for (int k = 0; k < 4; k++) { s6[k] = wg.r32(22 + 4 * k); d6[k] = wg.r32(38 + 4 * k); }
                    K[0] = K[1] = hz_key(s6, d6, 4, sp, dp, r.nh, di);           // the IPv6 path keeps its addresses
                    de = di;
                    K[2] = K[3] = hz_key(s6, d6, 4, 0u, 0u, 0x1ffu, pd);
                    K[4] = hz_key(s6, s6, 4, 0u, 0u, 0x2ffu, pd);
                    K[5] = hz_key(d6, d6, 4, 0u, 0u, 0x2ffu, pd);
                    const bool vip = !(r.eflags & GF_EG_F_LB) && vip6_has(E, d6);
                    const bool dlv = E.lxc.slots && lxc_has6(E.lxc, d6);
                    hfl = (r.nh == 58 ? GF_HZ_ICMP : 0u) | (vip ? GF_HZ_VIP : 0u) | GF_HZ_V6 | (dlv ? GF_HZ_DLV : 0u);
                } else {
                    const uint32_t sp = tu ? w.r16((uint32_t)lo4) : 0u, dp = tu ? w.r16((uint32_t)lo4 + 2u) : 0u;
                    const uint32_t fs = w.r32(26), fd = w.r32(30), ts = r.t_saddr, td = r.t_daddr;
                    K[0] = hz_key(&fs, &fd, 1, sp, dp, r.nh, di);
                    K[1] = hz_key(&ts, &td, 1, sp, dp, r.nh, de);
                    K[2] = hz_key(&fs, &fd, 1, 0u, 0u, 0x1ffu, pd);
                    K[3] = hz_key(&ts, &td, 1, 0u, 0u, 0x1ffu, pd);
                    K[4] = hz_key(&fs, &fs, 1, 0u, 0u, 0x2ffu, pd);
                    K[5] = hz_key(&fd, &fd, 1, 0u, 0u, 0x2ffu, pd);
                    const bool vip = !(r.eflags & GF_EG_F_LB) && vip4_has(E, fd);
                    const bool dlv = (E.lxc.slots && (E.lxset ? aset_has(E.lxset, E.lxbits, E.lxzero, fd) : lxc_has4(E.lxc, fd))) ||
                                     (E.loopback && fd == E.loopback);
                    hfl = (r.nh == 1 ? GF_HZ_ICMP : 0u) | (vip ? GF_HZ_VIP : 0u) |
                          ((r.eflags & GF_EG_F_LOOPBACK) ? GF_HZ_LOOP : 0u) | (dlv ? GF_HZ_DLV : 0u);
                }
                hfl |= GF_HZ_VALID | (di ? GF_HZ_DIRI : 0u) | (de ? GF_HZ_DIRE : 0u);
            }
            for (uint32_t k = 0; k < GF_HZ_NK; k++) E.hz_k[(size_t)k * fr.n + i] = K[k];
            E.hz_fl[i] = (uint8_t)hfl;
            if (hfl & (GF_HZ_ICMP | GF_HZ_VIP)) atomicOr(E.hz + 1, hfl);   // the batch's kinds
        }
        if (r.st == 0 && FAM == 6) {
            uint32_t s6[4], d6[4];
            for (int k = 0; k < 4; k++) { s6[k] = wg.r32(22 + 4 * k); d6[k] = wg.r32(38 + 4 * k); }
            key = gf_key_live(gf_pair_hash6(s6, d6), E.K) | E.K.fam;   // the IPv6 family of the schedule
        } else if (r.st == 0) {
            key = gf_key_live(gf_pair_hash4(r.t_saddr, r.t_daddr), E.K);
            if (E.conn) {
                E.keysP[i] = key;
                const bool tu = (r.nh == 6 || r.nh == 17) && skb_ok(r.l4_off, 4, len);
                const uint32_t sp = tu ? w.r16((uint32_t)r.l4_off) : 0u, dp = tu ? w.r16((uint32_t)r.l4_off + 2u) : 0u;
                key = gf_key_live(gf_conn_hash4(r.t_saddr, sp, r.t_daddr, dp, r.nh), E.K);
                if (r.nh == 1) atomicOr(E.cflag, 1u);
            }
            const uint32_t lo = E.loopback;
            if (r.t_saddr == r.t_daddr || (lo && (r.t_saddr == lo || r.t_daddr == lo)) || (E.strict & 1u)) *E.seq = 1u;
        } else {
            key = gf_key_skip(E.K);                   // final in the front: k_eg_groups has nothing to do
            if (E.conn) E.keysP[i] = key;
            if (o.stage == GF_STAGE_FROM_LXC) {
                if (ret < 0 || ret == TC_SHOT) {
                    o.action = TC_SHOT; o.reason = (uint8_t)(-ret);
                    o.eg_flags = r.eflags & (GF_EG_F_LB | GF_EG_F_LOOPBACK | GF_EG_F_PORTMAP | GF_EG_F_IPV6);
                    o.slave = r.slave; o.rev_nat = r.rev_nat;
                } else o.action = (uint8_t)ret;
            }
            out[i] = o;
            scnt = true; sreason = o.reason; saction = o.action; slen = len; sab = ab;
        }
        erec[i] = r;
        keys[i] = key;
        {                                                     // not (yet) a local delivery: skipped by the
            gf_rec rr;                                        // handle_policy pass (coalesced writes here,
            const uint32_t k2 = pack_rec(i, 0, len, 0, 0, 0, 0, 0, 0, 0, 0, r.ep, 0, true, false, nullptr, nullptr, rr, E.K);
            E.rec2[i] = rr;                                   // none for most packets in k_eg_groups)
            E.key2[i] = k2;
            if (E.conn) E.key2P[i] = k2;
        }
        if (FAM == 4 && !coop) eg_copy(dst, row, K);         // the frame as the front left it
    }
    if (coop) {             // every row of the block (IPv6 rows unchanged: k_eg_front<6> rewrites them after)
        __syncthreads();
        uint4 *g = reinterpret_cast<uint4 *>(E.snap + (size_t)b0 * S);
        for (uint32_t k = threadIdx.x; k < nv; k += BLOCK) g[k] = lds[k];
    }
    if (stats) { st.pkt_wave(scnt, sreason, saction, slen, sab); st.flush(stats); }
}

// After the front: a flagged batch runs as one bucket per family (every IPv4
// key equal; the IPv6 path writes no service entries and keeps its own bucket).
// With connection groups and an IPv4 ICMP packet in the run: the pair keys.
// The deliveries' keys of a run that fell back to pair groups (*cflag): their pair keys.
__global__ __launch_bounds__(BLOCK) void k_eg_pick_keys(const uint32_t *cflag, const uint32_t *key2P, uint32_t n,
                                                        uint32_t *keys) {
    if (!*cflag) return;
    for (uint32_t i = blockIdx.x * BLOCK + threadIdx.x; i < n; i += gridDim.x * BLOCK) keys[i] = key2P[i];
}
__global__ __launch_bounds__(BLOCK) void k_eg_seq_keys(const uint32_t *seq, const uint32_t *cflag,
                                                       const uint32_t *keysP, uint32_t n, uint32_t *keys,
                                                       gf_key_cfg K) {
    if (*seq) {
        for (uint32_t i = blockIdx.x * BLOCK + threadIdx.x; i < n; i += gridDim.x * BLOCK) keys[i] &= K.fam;
    } else if (cflag && *cflag) {
        for (uint32_t i = blockIdx.x * BLOCK + threadIdx.x; i < n; i += gridDim.x * BLOCK)
            if (!(keys[i] & K.fam)) keys[i] = keysP[i];
    }
}

// The ordering check: every continuing packet records the first batch index of
// its connection key per direction (open addressing, key 0 = empty)...
__device__ __forceinline__ void hz_put(unsigned long long k, uint32_t half, uint32_t i, unsigned long long *tkey,
                                       uint32_t *tfirst, uint32_t mask) {
    uint32_t slot = (uint32_t)(k >> 32) & mask;
    for (uint32_t probe = 0; probe <= mask; probe++) {
        const unsigned long long old = atomicCAS(&tkey[slot], 0ull, k);
        if (old == 0ull || old == k) { atomicMin(&tfirst[2 * slot + half], i); return; }
        slot = (slot + 1u) & mask;
    }
}
__device__ __forceinline__ uint32_t hz_get(unsigned long long k, uint32_t half, const unsigned long long *tkey,
                                           const uint32_t *tfirst, uint32_t mask) {
    uint32_t slot = (uint32_t)(k >> 32) & mask;
    for (uint32_t probe = 0; probe <= mask; probe++) {
        const unsigned long long t = tkey[slot];
        if (t == k) return tfirst[2 * slot + half];
        if (t == 0ull) break;
        slot = (slot + 1u) & mask;
    }
    return 0xffffffffu;
}
struct HzTab { unsigned long long *key; uint32_t *first; uint32_t mask; };
// The connection table is never cleared: a slot belongs to the current call when
// its key word carries the call's 16-bit generation (key = gen << 48 | 48 hash
// bits), and a first-index word is (gen << 32 | ~index), kept by atomicMax.  The
// host clears it when the generation wraps or the table is reallocated.
struct HzGen { unsigned long long *key; unsigned long long *first; uint32_t mask; uint32_t gen; };
__device__ __forceinline__ void hzg_put(const HzGen &T, unsigned long long k, uint32_t half, uint32_t i) {
    const unsigned long long want = ((unsigned long long)T.gen << 48) | (k & 0xffffffffffffull);
    uint32_t slot = (uint32_t)(k >> 32) & T.mask;
    for (uint32_t probe = 0; probe <= T.mask;) {
        unsigned long long cur = T.key[slot];
        if ((uint32_t)(cur >> 48) != T.gen) {          // a stale slot: claim it
            const unsigned long long old = atomicCAS(&T.key[slot], cur, want);
            if (old != cur) continue;                   // changed under us: look again
            cur = want;
        }
        if (cur == want) {
            atomicMax(&T.first[2 * slot + half], ((unsigned long long)T.gen << 32) | (0xffffffffull - i));
            return;
        }
        slot = (slot + 1u) & T.mask;
        probe++;
    }
}
__device__ __forceinline__ uint32_t hzg_get(const HzGen &T, unsigned long long k, uint32_t half) {
    const unsigned long long want = ((unsigned long long)T.gen << 48) | (k & 0xffffffffffffull);
    uint32_t slot = (uint32_t)(k >> 32) & T.mask;
    for (uint32_t probe = 0; probe <= T.mask; probe++) {
        const unsigned long long cur = T.key[slot];
        if ((uint32_t)(cur >> 48) != T.gen) break;
        if (cur == want) {
            const unsigned long long w = T.first[2 * slot + half];
            return (uint32_t)(w >> 32) == T.gen ? 0xffffffffu - (uint32_t)w : 0xffffffffu;
        }
        slot = (slot + 1u) & T.mask;
    }
    return 0xffffffffu;
}
// The pair / address keys live in a second table, cleared (here, on the device)
// only for a batch with ICMP or GF_HZ_VIP packets.
__global__ __launch_bounds__(BLOCK) void k_hz_clear(HzTab A, const uint32_t *hz) {
    if (!(hz[1] & (GF_HZ_ICMP | GF_HZ_VIP))) return;
    for (uint64_t k = blockIdx.x * (uint64_t)BLOCK + threadIdx.x; k <= A.mask; k += (uint64_t)gridDim.x * BLOCK) {
        A.key[k] = 0ull;
        A.first[2 * k] = A.first[2 * k + 1] = 0xffffffffu;
    }
}
__global__ __launch_bounds__(BLOCK) void k_hz_insert(const uint64_t *K, const uint8_t *fl, uint32_t n,
                                                     const uint32_t *hz, HzGen C, HzTab A) {
    const uint32_t kinds = hz[1];                       // pair / address keys only when a packet probes them
    for (uint32_t i = blockIdx.x * BLOCK + threadIdx.x; i < n; i += gridDim.x * BLOCK) {
        const uint32_t f = fl[i];
        if (!(f & GF_HZ_VALID)) continue;
        if (f & GF_HZ_DLV) hzg_put(C, K[i], (f & GF_HZ_DIRI) ? 1u : 0u, i);
        if (kinds & GF_HZ_ICMP) {
            hz_put(K[2ull * n + i], 0u, i, A.key, A.first, A.mask);
            if (f & GF_HZ_ICMP) hz_put(K[2ull * n + i] ^ GF_HZ_ICMPSALT, 0u, i, A.key, A.first, A.mask);
        }
        if (kinds & GF_HZ_VIP) {
            hz_put(K[4ull * n + i], 0u, i, A.key, A.first, A.mask);
            hz_put(K[5ull * n + i], 0u, i, A.key, A.first, A.mask);
        }
    }
}
// ... then each packet probes what its from-container part touches; a hit on an
// earlier index flags the batch.
__global__ __launch_bounds__(BLOCK) void k_hz_probe(const uint64_t *K, const uint8_t *fl, uint32_t n, HzGen C,
                                                    HzTab A, uint32_t strict, uint32_t *hz) {
    const uint32_t kinds = hz[1];
    bool hit = false, each = false;
    uint32_t first = 0xffffffffu;
    for (uint32_t i = blockIdx.x * BLOCK + threadIdx.x; i < n; i += gridDim.x * BLOCK) {
        const uint32_t f = fl[i];
        if (!(f & GF_HZ_VALID)) continue;
        each |= (strict & ((f & GF_HZ_V6) ? 2u : 1u)) != 0;
        hit |= hzg_get(C, K[1ull * n + i], (f & GF_HZ_DIRE) ? 0u : 1u) < i;
        if (kinds & GF_HZ_ICMP) {
            if (f & GF_HZ_ICMP) hit |= hz_get(K[3ull * n + i], 0u, A.key, A.first, A.mask) < i;
            hit |= hz_get(K[3ull * n + i] ^ GF_HZ_ICMPSALT, 0u, A.key, A.first, A.mask) < i;
        }
        if (f & GF_HZ_LOOP)
            hit |= hzg_get(C, K[i], 0u) < i || hzg_get(C, K[i], 1u) < i;
        if (f & GF_HZ_VIP) hit |= hz_get(K[4ull * n + i], 0u, A.key, A.first, A.mask) < i;
        if (hit && first == 0xffffffffu) first = i;
    }
    // the earliest flagged packet: everything before it is a run without a hazard
    uint32_t m = first;
    for (int o = 32; o > 0; o >>= 1) m = min(m, (uint32_t)__shfl_xor(m, o));
    if ((threadIdx.x & 63u) == 0 && m != 0xffffffffu) atomicMin(hz + 2, m);
    if (__any(each) && (threadIdx.x & 63u) == 0) atomicOr(hz, 2u);
    else if (__any(hit) && (threadIdx.x & 63u) == 0) atomicOr(hz, 1u);
}

// Adds a call's counter block to the registered sink.
__global__ void k_stats_fold(const unsigned long long *src, unsigned long long *dst) {
    for (int k = threadIdx.x; k < 272; k += blockDim.x)
        if (src[k]) atomicAdd(&dst[k], src[k]);
}

// __ct_lookup hit part for CT_EGRESS (conntrack.h:75-135): tx accounting (the
// cold part of the value), TX_CLOSING on close.
__device__ __forceinline__ void ct_hit_eg(const gf_htab_desc &d, int64_t f, int action, bool syn, uint32_t len,
                                          uint32_t now, bool acct, CtState &st) {
    uint8_t *e = ht_val(d, (uint64_t)f);
    uint4 hot = gload<uint4>(e);
    uint32_t life = hot.x, fl = hot.y & 0xffffu;
    if (!(fl & F_RX_CLOSING) || !(fl & F_TX_CLOSING)) {
        if (!syn) fl |= F_SEEN_NON_SYN;
        life = now + ((fl & F_SEEN_NON_SYN) ? 43200u : 300u);
    }
    st.rev_nat = hot.y >> 16;
    st.loopback = (fl >> 3) & 1u;
    if (acct) {                                         // tx_packets += 1, tx_bytes += len
        uint8_t *base = d.sstride ? ht_side(d, (uint64_t)f) - 16 : e;   // internal value word k at base + 4k
        gstore<unsigned long long>(base + 24, gload<unsigned long long>(base + 24) + 1ull);
        gstore<unsigned long long>(base + 32, gload<unsigned long long>(base + 32) + (unsigned long long)len);
    }
    if (action == ACT_CREATE) {
        if (fl & (F_RX_CLOSING | F_TX_CLOSING)) {
            fl &= ~(F_RX_CLOSING | F_TX_CLOSING);
            if (!syn) fl |= F_SEEN_NON_SYN;
            life = now + ((fl & F_SEEN_NON_SYN) ? 43200u : 300u);
        }
    } else if (action == ACT_CLOSE) {
        fl |= F_TX_CLOSING;
        if ((fl & F_RX_CLOSING) && (fl & F_TX_CLOSING)) life = now + 10u;
    }
    hot.x = life;
    hot.y = (hot.y & 0xffff0000u) | fl;
    gstore<uint4>(e, hot);
    GF_WR(WR_HIT);
}

// policy_can_egress4 (policy.h:241-264 with POLICY_EGRESS, else :282-289):
// ipcache identity, __policy_can_access(dir = CT_EGRESS: key.egress = 1, the
// CFG_L3L4_EGRESS list), reserved identities through CIDR4_EGRESS_MAP.
__device__ __forceinline__ int eg_policy(const gf_lxc_dev *c, uint32_t flags, uint32_t dst_id, const uint32_t *da, bool v6,
                         uint32_t dport, uint32_t proto, uint32_t len, uint32_t &ab) {
    if (flags & GF_LXC_F_DROP_ALL) return D_POLICY;
    if (!(flags & GF_LXC_F_POLICY_EGRESS)) return TC_OK;
    uint32_t identity = dst_id;
    const gf_htab_desc ic = gload<gf_htab_desc>(&c->ipcache);
    if (ic.slots) {
        uint32_t kw[5] = {da[0], v6 ? da[1] : 0u, v6 ? da[2] : 0u, v6 ? da[3] : 0u, v6 ? 2u : 1u};
        const int64_t f = ht_find<20>(ic, kw, key_hash<20>(kw));
        ab += 20;
        if (f >= 0) { identity = gload<uint16_t>(ht_val(ic, f)); ab += 8; }
    }
    const gf_htab_desc pd = gload<gf_htab_desc>(&c->policy);
    int verdict = D_POLICY;
    int64_t f = -1;
    bool l4hit = false;
    if (flags & GF_LXC_F_HAVE_L4_POLICY) {
        uint32_t kw[2] = {identity, dport | (proto << 16) | (1u << 24)};
        f = ht_find<8, GF_POL_U>(pd, kw, key_hash<8, GF_HASH_POLICY>(kw));
        ab += 8;
        l4hit = f >= 0;
    }
    if (f < 0) {
        uint32_t kw[2] = {identity, 1u << 24};
        f = ht_find<8, GF_POL_U>(pd, kw, key_hash<8, GF_HASH_POLICY>(kw));
        ab += 8;
        if (f >= 0) verdict = TC_OK;
    }
    if (f < 0 && (flags & GF_LXC_F_HAVE_L4_POLICY)) {
        uint32_t kw[2] = {0u, dport | (proto << 16) | (1u << 24)};
        f = ht_find<8, GF_POL_U>(pd, kw, key_hash<8, GF_HASH_POLICY>(kw));
        ab += 8;
        l4hit = f >= 0;
    }
    if (f >= 0) {
        uint8_t *cnt = pd.vals + (uint64_t)f * GF_POL_SIDE;          // packets / bytes (policy.h:67-92)
        pol_count_add(cnt, 1u, len, false);
        ab += 40;
        if (l4hit) {
            const uint32_t pp = gload<uint16_t>(ht_val(pd, (uint64_t)f));
            verdict = 0;
            if (pp) verdict = (int)pp;
            else if (proto == 6 || proto == 17) {         // l4_egress_proxy_lookup (l4.h:178-188)
                const uint32_t n = gload<uint32_t>(&c->n_l4e);
                for (uint32_t k = 0; k < n; k++) {
                    const gf_l4_allow_dev a = gload<gf_l4_allow_dev>(&c->l4e[k]);
                    if (a.port && a.port == dport) { if (a.nexthdr && a.nexthdr == proto) { verdict = a.proxy; break; } }
                }
            }
        }
    }
    if (identity < 256 && verdict < 0) {               // identity_is_reserved -> lpm{4,6}_egress_lookup
        const gf_trie_desc tr = gload<gf_trie_desc>(v6 ? &c->cidr6e : &c->cidr4e);
        if (tr.root_bits) ab += v6 ? 21 : 9;
        verdict = (v6 ? trie_lookup<4>(tr, da) : trie_lookup<1>(tr, da)) ? 0 : D_POLICY_CIDR;
    }
    return verdict;
}

// The from-container program's CT map (CT_MAP4 / CT_MAP6 of the sending endpoint):
// the global one of the launch, or (PCT, ConntrackLocal) the program's own.
template <int FAM, bool PCT>
__device__ __forceinline__ gf_htab_desc eg_ct(const EgDev &E, const gf_lxc_dev *c) {
    if constexpr (PCT) return gload<gf_htab_desc>(FAM == 6 ? &c->ct6 : &c->ct4);
    else return FAM == 6 ? E.ct6 : E.ct4;
}

// The CT / policy part of handle_ipv4_from_lxc (bpf_lxc.c:499-658) for packet i.
// Returns TC_OK / TC_REDIRECT / ND_TAILCALL (local delivery; ifx, lxc, mapped
// filled) or an error.
template <bool PCT>
__device__ __forceinline__ int eg_ct_part(const EgDev &E, const EgRec &r, uint32_t i, Row &w, gf_egress_out &o, uint32_t &ifx,
                          uint32_t &lxc, int *added, bool seq, bool rlog, uint32_t &ab) {
    const uint32_t len = r.len, nh = r.nh;
    const int l4_off = r.l4_off;
    const gf_lxc_dev *c = E.cfgs + (r.ep - 1);
    const uint32_t flags = gload<uint32_t>(&c->flags);
    const uint32_t co = csum_l4_offset(nh), fl = nh == 17 ? GF_F_MANGLED_0 : 0u;
    // ct_lookup4(CT_EGRESS): the L4 words as the frame holds them now
    gf_rec hr{};
    hr.len = len; hr.l4_off = (int16_t)l4_off;
    for (int k = 0; k < 4; k++) { const int64_t off = (int64_t)l4_off + k; if (off >= 0 && off < (int64_t)len) hr.l4w0 |= w.b((uint32_t)off) << (8 * k); }
    {
        uint32_t w3 = 0;
        for (int k = 0; k < 2; k++) { const int64_t off = (int64_t)l4_off + 12 + k; if (off >= 0 && off < (int64_t)len) w3 |= w.b((uint32_t)off) << (8 * k); }
        hr.l4w3 = (uint16_t)w3;
    }
    uint32_t t[4] = {r.t_daddr, r.t_saddr, 0u, nh};
    uint32_t tfl = 1u;                                  // TUPLE_F_IN (egress)
    int action; bool syn;
    int e = ct_l4(nh, false, hr, t[2], tfl, action, syn);
    if (e < 0) return e;
    t[3] = nh | (tfl << 8);
    if (!(flags & GF_LXC_DEV_HAS_CT4)) return D_CT_CREATE_FAILED;   // (no CT map bound: never in a valid config)
    const gf_htab_desc ct = eg_ct<4, PCT>(E, c);
    const bool acct = (flags & GF_LXC_F_CT_ACCOUNTING) != 0;
    uint32_t tf[4] = {t[1], t[0], (t[2] >> 16) | (t[2] << 16), nh | ((tfl ^ 1u) << 8)};
    bool isb = false;
#if GF_EG_COOP
    // the home line read by the lane quad together (the egress CT4 holds 2^28 slots, 8 GB)
    ProbeLine<14, GF_CT4_U, 4> cl;
    cl.load_quad(ct, key_hash<14, GF_HASH_CT>(t));
    const ProbeRes pr = probe2<14, GF_CT4_U, 4>(ct, t, tf, cl, true);
    const int64_t f = pr.f;
    isb = pr.is_b;
#else
    const int64_t f = ht_find2<14, GF_CT4_U>(ct, t, tf, key_hash<14, GF_HASH_CT>(t), &isb);
#endif
    ab += 14;
    CtState st{0, 0, 0};
    int ret;
    if (f >= 0 && !isb) {
        ab += 96;
        ct_hit_eg(ct, f, action, syn, len, E.now, acct, st);
        ret = (tfl & 2u) ? CT_RELATED : CT_REPLY;
    } else {
        ab += 14;
        for (int k = 0; k < 4; k++) t[k] = tf[k];
        tfl ^= 1u;
        if (f >= 0) { ab += 96; ct_hit_eg(ct, f, action, syn, len, E.now, acct, st); ret = CT_ESTABLISHED; }
        else ret = CT_NEW;
    }
    o.eg_ct_ret = (uint8_t)ret;
    const uint32_t dst_id = ((r.orig_dip & E.cluster_mask) == E.cluster_range) ? 3u : 2u;   // CLUSTER_ID / WORLD_ID
    if (E.X.tmark && dst_id == 3u) E.X.tmark[i] |= GF_TR_CLUSTER;
    const int verdict = eg_policy(c, flags, dst_id, &t[1], false, t[2] & 0xffffu, nh, len, ab);
    if (ret != CT_REPLY && ret != CT_RELATED && verdict < 0) {
        if (ret == CT_ESTABLISHED) {
            ab += 14;
            ht_delete<14, GF_HASH_CT, GF_CT4_U>(ct, t, (E.strict & 1) != 0, added);
            o.eg_flags |= GF_EG_F_DELETED;
        }
        return verdict;
    }
    if (ret == CT_NEW) {                                // ct_create4(CT_EGRESS), conntrack.h:503-580
        ab += 3 * (14 + 48);
        const uint32_t loop = (r.eflags & GF_EG_F_LOOPBACK) ? 1u : 0u;
        uint32_t efl = (nh == 6) ? 0u : F_SEEN_NON_SYN;
        efl |= loop ? F_LB_LOOPBACK : 0u;
        const uint32_t life = E.now + ((efl & F_SEEN_NON_SYN) ? 43200u : 300u);
        const uint32_t seclabel = gload<uint32_t>(&c->seclabel);
        // GF_VCODEC_CT: lifetime, flags|rev_nat, rx lo x2, rx hi x2, tx_packets, tx_bytes, unused, src_sec_id
        uint32_t v[12] = {life, efl | ((uint32_t)r.rev_nat << 16), 0u, 0u, 0u, 0u, 1u, 0u, len, 0u, 0u, seclabel};
        const bool strict = (E.strict & 1) != 0;
        if (ht_upsert<14, 12, GF_HASH_CT, GF_CT4_U>(ct, t, v, strict, added) < 0) return D_CT_CREATE_FAILED;
        if (r.ct_addr) {
            uint32_t t2[4] = {r.ct_addr, t[1], t[2], t[3]};          // dir EGRESS: tuple->daddr = ct_state->addr
            if (loop) { t2[3] = nh | (1u << 8); t2[1] = r.t_saddr; }  // TUPLE_F_IN, tuple->saddr = svc_addr
            if (seq) {
                if (ht_upsert<14, 12, GF_HASH_CT, GF_CT4_U>(ct, t2, v, strict, added) < 0) return D_CT_CREATE_FAILED;
            } else {
                uint32_t *lg = E.ctlog + (size_t)GF_CTLOG_WORDS * atomicAdd(E.ctlog_n, 1u);
                lg[0] = i;
                for (int k = 0; k < 4; k++) lg[1 + k] = t2[k];
                for (int k = 0; k < 12; k++) lg[5 + k] = v[k];
                if constexpr (PCT) {                    // the entry's map: its program and its slot array
                    lg[17] = r.ep;
                    lg[18] = (uint32_t)(uintptr_t)ct.slots; lg[19] = (uint32_t)((uintptr_t)ct.slots >> 32);
                }
            }
        }
        uint32_t it[4] = {t[0], t[1], 0u, 1u | ((((t[3] >> 8) & 0xffu) | 2u) << 8)};
        v[1] |= F_SEEN_NON_SYN;
        if (rlog && E.rs.slot) {                        // the run's set (RelSet), applied after the run
            rset_put(E.rs, it[0], it[1], (it[3] >> 8) & 1u, 2u * i);
        } else if (rlog) {                              // applied after the run, in packet order (the pair's
            uint32_t *lg = E.rlog + (size_t)GF_CTLOG_WORDS * wave_reserve(E.rlog_n);   // other connections
            lg[0] = 2u * i;                                                             // never read it)
            for (int k = 0; k < 4; k++) lg[1 + k] = it[k];
            for (int k = 0; k < 12; k++) lg[5 + k] = v[k];
        } else if (ht_upsert<14, 12, GF_HASH_CT, GF_CT4_U>(ct, it, v, strict, added) < 0) {
            return D_CT_CREATE_FAILED;
        }
        o.eg_flags |= GF_EG_F_CREATED;
    } else if (ret == CT_REPLY || ret == CT_RELATED) {
        if (st.rev_nat) {                               // lb4_rev_nat(flags 0), lb.h:447-534
            const gf_htab_desc rn = gload<gf_htab_desc>(&c->revnat4);
            uint32_t kw[1] = {st.rev_nat};
            const int64_t fr_ = ht_find<2>(rn, kw, key_hash<2>(kw));
            ab += 8;
            if (fr_ >= 0) {
                const uint8_t *nat = ht_val(rn, fr_);
                const uint32_t port = gload<uint16_t>(nat + 4);
                if (port) {                             // reverse_map_l4_port
                    if (nh == 6 || nh == 17) {
                        if (!skb_ok(l4_off, 2, len)) return -GF_EFAULT;
                        const uint32_t old = w.r16((uint32_t)l4_off);
                        if (port != old) {
                            if (l4_csum(w, len, l4_off + (int)co, old, port, 2u | fl) < 0) return D_CSUM_L4;
                            if (!skb_ok(l4_off, 2, len)) return D_WRITE_ERROR;
                            w.w16((uint32_t)l4_off, port);
                        }
                    } else if (nh != 1 && nh != 58) return D_UNKNOWN_L4;
                }
                const uint32_t old_sip = w.r32(26), new_sip = gload<uint32_t>(nat);
                uint32_t sum = 0;
                if (st.loopback) {
                    const uint32_t old_dip = w.r32(30);
                    w.w32(30, old_sip);
                    sum = ck_add(ck_add(0u, ~old_dip), old_sip);
                    t[1] = old_sip;
                }
                w.w32(26, new_sip);
                sum = ck_add(sum, ck_add(ck_add(0u, ~old_sip), new_sip));
                l3_csum(w, len, 24, 0, sum, 0);
                if (co && l4_csum(w, len, l4_off + (int)co, 0, sum, GF_F_PSEUDO_HDR | fl) < 0) return D_CSUM_L4;
                ab += 16;
            }
            o.eg_flags |= GF_EG_F_REVNAT;
        }
    }
    uint32_t nm[2] = {gload<uint32_t>(&c->node_mac[0]), gload<uint32_t>(&c->node_mac[1])};
    if (verdict > 0) {                                  // ipv4_redirect_to_host_port + ipv4_l3 -> HOST_IFINDEX
        if (E.X.tmark)
            trace_proxy(E.X.tmark, E.X.tcap, E.snap + (size_t)i * E.stride, w.p, w.cap, trace_cap_len(len, E.stride), i,
                        GF_TR_PX_EGRESS);
        const int r3 = redirect_checks(len, l4_off, nh);
        if (r3 < 0) return r3;
        const uint32_t od[1] = {r.orig_dip};
        const uint32_t np = (uint32_t)verdict & 0xffffu, gw = E.X.gw;
        l4_csum(w, len, l4_off + (int)co, t[2] & 0xffffu, np, 2u | fl);   // l4_modify_port (lxc.h:124)
        w.w16((uint32_t)(l4_off + 2), np);
        w.w32(30, gw);                                                    // daddr = IPV4_GATEWAY
        l3_csum(w, len, 24, r.orig_dip, gw, 4);
        if (co) l4_csum(w, len, l4_off + (int)co, r.orig_dip, gw, 4u | GF_F_PSEUDO_HDR | fl);
        pol_redirect(E.X, i, len, l4_off, nh, t, false, np, od, gload<uint32_t>(&c->seclabel), 1u);
        o.eg_flags |= GF_EG_F_PROXY;
        o.proxy_port = (uint16_t)verdict;
        const int r4 = eg_ipv4_l3(w, len, nm, E.host_mac);
        if (r4 != TC_OK) return r4;
        ifx = E.host_ifindex;
        return TC_REDIRECT;
    }
    const uint32_t dip = w.r32(30);
    if (E.lxc.slots) {                                  // lookup_ip4_endpoint
        uint32_t kw[5] = {dip, 0, 0, 0, 1u};
        const int64_t fe = E.lxset ? aset_slot(E.lxset, E.lxbits, E.lxzero, dip) : ht_find<20>(E.lxc, kw, key_hash<20>(kw));
        ab += 20;
        if (fe >= 0) {
            const uint8_t *ep = ht_val(E.lxc, fe);
            ab += 8;
            if (gload<uint32_t>(ep + 8) & 1u) {         // ENDPOINT_F_HOST -> to_host
                if (!E.host_ifindex) return D_NO_LXC;
                const int r4 = eg_ipv4_l3(w, len, nm, E.host_mac);
                if (r4 != TC_OK) return r4;
                o.eg_flags |= GF_EG_F_TO_HOST;
                ifx = E.host_ifindex;
                return TC_REDIRECT;
            }
            // ipv4_local_delivery (l3.h:136-168): ipv4_l3(node_mac, mac), map_lxc_in, tail call
            const uint32_t ttl = w.b(22);
            if (ttl <= 1) return D_INVALID;
            l3_csum(w, len, 24, ttl, ttl - 1, 2);
            w.w8(22, ttl - 1);
            o.eg_flags |= GF_EG_F_LOCAL;
            uint32_t mapped = 0, ndport = 0;
            return delivery_tail(w, len, l4_off, nh, ep, ifx, lxc, mapped, ndport, ab);
        }
    }
    if (E.encap_ifindex && E.tunnel.slots) {            // encap_and_redirect (lib/encap.h)
        uint32_t kw[5] = {dip & E.ipv4_mask, 0, 0, 0, 1u};
        const int64_t ft = E.tnset ? aset_slot(E.tnset, E.tnbits, E.tnzero, kw[0]) : ht_find<20>(E.tunnel, kw, key_hash<20>(kw));
        ab += 20;
        if (ft >= 0) {
            o.tunnel_ip = __builtin_bswap32(gload<uint32_t>(ht_val(E.tunnel, ft)));
            o.eg_flags |= GF_EG_F_ENCAP;
            ifx = E.encap_ifindex;
            ab += 20;
            return TC_REDIRECT;
        }
    }
    const int r4 = eg_ipv4_l3(w, len, nullptr, nm);    // pass_to_stack
    if (r4 != TC_OK) return r4;
    o.eg_flags |= GF_EG_F_TO_STACK;
    return TC_OK;
}

// ipv6_l3 (bpf/lib/l3.h:31-52) + ipv6_dec_hoplimit (bpf/lib/ipv6.h:178-193); smac may
// be null.  ND_ICMP6_TE: the hop limit ran out (icmp6_send_time_exceeded).
__device__ __forceinline__ int eg_ipv6_l3(Row &w, const uint32_t *smac, const uint32_t *dmac) {
    const uint32_t hl = w.b(21);
    if (hl <= 1) return ND_ICMP6_TE;
    w.w8(21, hl - 1);
    if (smac) { w.w32(6, smac[0]); w.w16(10, smac[1] & 0xffffu); }
    w.w32(0, dmac[0]); w.w16(4, dmac[1] & 0xffffu);
    return TC_OK;
}

// The CT / policy part of ipv6_l3_from_lxc (bpf_lxc.c:186-386) for packet i, on
// the frame in HBM (extension headers may put the L4 header anywhere in the snap).
template <bool PCT>
__device__ __forceinline__ int eg_ct_part6(const EgDev &E, const EgRec &r, uint32_t i, Row &w, gf_egress_out &o,
                                           uint32_t &ifx, uint32_t &lxc, int *added, uint32_t &ab) {
    const uint32_t len = r.len, nh = r.nh;
    const int l4_off = r.l4_off;
    const gf_lxc_dev *c = E.cfgs + (r.ep - 1);
    const uint32_t flags = gload<uint32_t>(&c->flags);
    const uint32_t co = csum_l4_offset(nh), fl = nh == 17 ? GF_F_MANGLED_0 : 0u;
    gf_rec hr{};
    hr.len = len; hr.l4_off = (int16_t)l4_off;
    for (int k = 0; k < 4; k++) { const int64_t off = (int64_t)l4_off + k; if (off >= 0 && off < (int64_t)len) hr.l4w0 |= w.b((uint32_t)off) << (8 * k); }
    {
        uint32_t w3 = 0;
        for (int k = 0; k < 2; k++) { const int64_t off = (int64_t)l4_off + 12 + k; if (off >= 0 && off < (int64_t)len) w3 |= w.b((uint32_t)off) << (8 * k); }
        hr.l4w3 = (uint16_t)w3;
    }
    uint32_t t[10];
    for (int k = 0; k < 4; k++) { t[k] = w.r32(38 + 4 * k); t[4 + k] = w.r32(22 + 4 * k); }
    const uint32_t od[4] = {t[0], t[1], t[2], t[3]};   // orig_dip (after lb6_local)
    t[8] = 0; t[9] = nh;
    uint32_t tfl = 1u;                                  // TUPLE_F_IN (egress)
    int action; bool syn;
    int e = ct_l4(nh, true, hr, t[8], tfl, action, syn);
    if (e < 0) return e;
    t[9] = nh | (tfl << 8);
    if (!(flags & GF_LXC_DEV_HAS_CT6)) return D_CT_CREATE_FAILED;
    const gf_htab_desc ct = eg_ct<6, PCT>(E, c);
    const bool acct = (flags & GF_LXC_F_CT_ACCOUNTING) != 0;
    uint32_t tf[10];
    for (int k = 0; k < 4; k++) { tf[k] = t[4 + k]; tf[4 + k] = t[k]; }
    tf[8] = (t[8] >> 16) | (t[8] << 16);
    tf[9] = nh | ((tfl ^ 1u) << 8);
    bool isb = false;
    const int64_t f = ht_find2<40, GF_CT6_U>(ct, t, tf, key_hash<40, GF_HASH_CT>(t), &isb);
    ab += 40;
    CtState st{0, 0, 0};
    int ret;
    if (f >= 0 && !isb) {
        ab += 96;
        ct_hit_eg(ct, f, action, syn, len, E.now, acct, st);
        ret = (tfl & 2u) ? CT_RELATED : CT_REPLY;
    } else {
        ab += 40;
        for (int k = 0; k < 10; k++) t[k] = tf[k];
        tfl ^= 1u;
        if (f >= 0) { ab += 96; ct_hit_eg(ct, f, action, syn, len, E.now, acct, st); ret = CT_ESTABLISHED; }
        else ret = CT_NEW;
    }
    o.eg_ct_ret = (uint8_t)ret;
    const uint32_t dst_id = (w.r32(38) == E.router6[0] && w.r32(42) == E.router6[1]) ? 3u : 2u;
    if (E.X.tmark && dst_id == 3u) E.X.tmark[i] |= GF_TR_CLUSTER;
    const int verdict = eg_policy(c, flags, dst_id, &t[4], true, t[8] & 0xffffu, nh, len, ab);
    const bool strict = (E.strict & 2) != 0;
    if (ret != CT_REPLY && ret != CT_RELATED && verdict < 0) {
        if (ret == CT_ESTABLISHED) {
            ab += 40;
            ht_delete<40, GF_HASH_CT, GF_CT6_U>(ct, t, strict, added);
            o.eg_flags |= GF_EG_F_DELETED;
        }
        return verdict;
    }
    if (ret == CT_NEW) {                                // ct_create6(CT_EGRESS), conntrack.h:446-493
        ab += 2 * (40 + 48);
        const uint32_t efl = (nh == 6) ? 0u : F_SEEN_NON_SYN;
        const uint32_t life = E.now + ((efl & F_SEEN_NON_SYN) ? 43200u : 300u);
        uint32_t v[12] = {life, efl | ((uint32_t)r.rev_nat << 16), 0u, 0u, 0u, 0u, 1u, 0u, len, 0u, 0u,
                          gload<uint32_t>(&c->seclabel)};
        if (ht_upsert<40, 12, GF_HASH_CT, GF_CT6_U>(ct, t, v, strict, added) < 0) return D_CT_CREATE_FAILED;
        uint32_t it[10];
        for (int k = 0; k < 8; k++) it[k] = t[k];
        it[8] = 0;
        it[9] = 58u | ((((t[9] >> 8) & 0xffu) | 2u) << 8);
        v[1] |= F_SEEN_NON_SYN;
        if (ht_upsert<40, 12, GF_HASH_CT, GF_CT6_U>(ct, it, v, strict, added) < 0) return D_CT_CREATE_FAILED;
        o.eg_flags |= GF_EG_F_CREATED;
    } else if ((ret == CT_REPLY || ret == CT_RELATED) && st.rev_nat) {   // lb6_rev_nat(flags 0)
        const gf_htab_desc rn = gload<gf_htab_desc>(&c->revnat6);
        uint32_t kw[1] = {st.rev_nat};
        const int64_t fr_ = ht_find<2>(rn, kw, key_hash<2>(kw));
        ab += 20;
        if (fr_ >= 0) {
            const uint8_t *nat = ht_val(rn, fr_);
            const uint32_t port = gload<uint16_t>(nat + 16);
            if (port) {
                if (nh == 6 || nh == 17) {
                    if (!skb_ok(l4_off, 2, len)) return -GF_EFAULT;
                    const uint32_t old = w.r16((uint32_t)l4_off);
                    if (port != old) {
                        if (l4_csum(w, len, l4_off + (int)co, old, port, 2u | fl) < 0) return D_CSUM_L4;
                        if (!skb_ok(l4_off, 2, len)) return D_WRITE_ERROR;
                        w.w16((uint32_t)l4_off, port);
                    }
                } else if (nh != 1 && nh != 58) return D_UNKNOWN_L4;
            }
            uint32_t sum = 0;
            for (int k = 0; k < 4; k++) {
                const uint32_t os = w.r32(22 + 4 * k), nw = gload<uint32_t>(nat + 4 * k);
                w.w32(22 + 4 * k, nw);
                sum = ck_add(ck_add(sum, ~os), nw);
            }
            if (l4_csum(w, len, l4_off + (int)co, 0, sum, GF_F_PSEUDO_HDR | fl) < 0) return D_CSUM_L4;
        }
        o.eg_flags |= GF_EG_F_REVNAT;
    }
    uint32_t nm[2] = {gload<uint32_t>(&c->node_mac[0]), gload<uint32_t>(&c->node_mac[1])};
    if (verdict > 0) {                                  // ipv6_redirect_to_host_port + ipv6_l3 -> HOST_IFINDEX
        if (E.X.tmark)
            trace_proxy(E.X.tmark, E.X.tcap, w.p, nullptr, 0, trace_cap_len(len, E.stride), i, GF_TR_PX_EGRESS);
        const int r3 = redirect_checks(len, l4_off, nh);
        if (r3 < 0) return r3;
        const uint32_t np = (uint32_t)verdict & 0xffffu;
        l4_csum(w, len, l4_off + (int)co, t[8] & 0xffffu, np, 2u | fl);   // l4_modify_port
        w.w16((uint32_t)(l4_off + 2), np);
        uint32_t sum = 0;
        for (int k = 0; k < 4; k++) { w.w32(38 + 4 * k, E.host6[k]); sum = ck_add(ck_add(sum, ~od[k]), E.host6[k]); }
        if (co) l4_csum(w, len, l4_off + (int)co, 0, sum, GF_F_PSEUDO_HDR | fl);
        pol_redirect(E.X, i, len, l4_off, nh, t, true, np, od, gload<uint32_t>(&c->seclabel), 1u);
        o.eg_flags |= GF_EG_F_PROXY;
        o.proxy_port = (uint16_t)verdict;
        const int r4 = eg_ipv6_l3(w, nm, E.host_mac);
        if (r4 != TC_OK) return r4;
        ifx = E.host_ifindex;
        return TC_REDIRECT;
    }
    uint32_t d6[4];
    for (int k = 0; k < 4; k++) d6[k] = w.r32(38 + 4 * k);
    if (E.lxc.slots) {                                  // lookup_ip6_endpoint
        uint32_t kw[5] = {d6[0], d6[1], d6[2], d6[3], 2u};
        const int64_t fe = ht_find<20>(E.lxc, kw, key_hash<20>(kw));
        ab += 20;
        if (fe >= 0) {
            const uint8_t *ep = ht_val(E.lxc, fe);
            ab += 8;
            if (gload<uint32_t>(ep + 8) & 1u) {         // ENDPOINT_F_HOST -> to_host
                if (!E.host_ifindex) return D_NO_LXC;
                const int r4 = eg_ipv6_l3(w, nm, E.host_mac);
                if (r4 != TC_OK) return r4;
                o.eg_flags |= GF_EG_F_TO_HOST;
                ifx = E.host_ifindex;
                return TC_REDIRECT;
            }
            uint32_t emac[2] = {gload<uint32_t>(ep + 16), gload<uint32_t>(ep + 20)};
            uint32_t rmac[2] = {gload<uint32_t>(ep + 24), gload<uint32_t>(ep + 28)};
            const int r4 = eg_ipv6_l3(w, rmac, emac);   // ipv6_local_delivery (l3.h:106-134)
            if (r4 != TC_OK) return r4;
            o.eg_flags |= GF_EG_F_LOCAL;
            uint32_t mapped = 0, ndport = 0;
            return delivery_tail(w, len, l4_off, nh, ep, ifx, lxc, mapped, ndport, ab);
        }
    }
    if (E.encap_ifindex && E.tunnel.slots) {            // encap_and_redirect, key daddr/96
        uint32_t kw[5] = {d6[0], d6[1], d6[2], 0u, 2u};
        const int64_t ft = ht_find<20>(E.tunnel, kw, key_hash<20>(kw));
        ab += 20;
        if (ft >= 0) {
            o.tunnel_ip = __builtin_bswap32(gload<uint32_t>(ht_val(E.tunnel, ft)));
            o.eg_flags |= GF_EG_F_ENCAP;
            ifx = E.encap_ifindex;
            return TC_REDIRECT;
        }
    }
    const int r4 = eg_ipv6_l3(w, nullptr, nm);         // pass_to_stack
    if (r4 != TC_OK) return r4;
    {                                                   // ipv6_store_flowlabel(SECLABEL_NB), ipv6.h:245-260
        const uint32_t old = w.r32(14) & __builtin_bswap32(0x0FF00000u);
        w.w32(14, __builtin_bswap32(0x60000000u) | __builtin_bswap32(gload<uint32_t>(&c->seclabel)) | old);
    }
    o.eg_flags |= GF_EG_F_TO_STACK;
    return TC_OK;
}

// One bucket per lane from the longest-first queue (the ingress schedule), in
// batch order.  Writes each packet's verdict, and for local deliveries the
// handle_policy record + flow-group key of the ingress pass (rec2 / key2).
// FAM 4 runs the schedule's family 0 (IPv4 buckets and every packet the front
// finished), FAM 6 family 1 (IPv6); the two touch disjoint state.
// PCT: per-endpoint CT maps (ConntrackLocal): each packet's net element change goes
// to its own program's map as the packet ends (ct_count unused).
template <int FAM, bool PCT = false>
__global__ __launch_bounds__(BLOCK, GF_EG_MINW) void k_eg_groups(EgDev E, uint32_t *sched, const uint2 *order, const uint32_t *perm,
                                                     const EgRec *erec, gf_egress_out *out, gf_rec *rec2, uint32_t *key2,
                                                     uint32_t *ct_count, unsigned long long *stats) {
    if (E.hz && *E.hz) return;                          // hazard: the batch reruns in ordered runs
    if (!GF_SCHED_NFAM(sched)[FAM == 6 ? 1 : 0]) return;   // no bucket of this family (nothing to count)
    __shared__ uint32_t sl[272];
    __shared__ uint32_t sadd;
    // FAM 4: one LDS row per lane of the staged header bytes, sized by the snap
    // (eg_row_bytes: 64-B snaps take half the LDS of 128-B rows, so more blocks
    // fit a CU — the LDS, not the registers, bounded the waves); FAM 6: unused
    extern __shared__ uint4 lds[];
    __shared__ uint32_t lsum[3 * BLOCK];                // the lane's packets / wire bytes / algorithmic bytes
    Stats st{sl};
    uint32_t *ls = lsum + 3 * threadIdx.x;
    ls[0] = ls[1] = ls[2] = 0;
    auto fold = [&]() { st.add_n(268, ls[0]); st.add_n(269, ls[1]); st.add_n(270, ls[2]); ls[0] = ls[1] = ls[2] = 0; };
    if (threadIdx.x == 0) sadd = 0;
    if (stats) st.init(); else __syncthreads();
    const uint32_t K = eg_stage_bytes(E.stride);
    uint8_t *row = reinterpret_cast<uint8_t *>(lds) + (FAM == 6 ? 0 : threadIdx.x * eg_row_bytes(E.stride));
    constexpr int F = FAM == 6 ? 1 : 0;
    const uint32_t nb = GF_SCHED_LCNT(sched)[F], lane = threadIdx.x & 63u;
    uint32_t *queue = GF_SCHED_QUEUE(sched) + F;
    order += GF_SCHED_LSTART(sched)[F];
    const bool seq = *E.seq != 0;
    const bool rlog = FAM == 4 && E.conn && !seq && !*E.cflag;   // connection groups: related entries logged
    int added = 0;
    // the wave's grab: [base, base + 64 * left) of the list, one 64-bucket round at a
    // time (wave-uniform values); grab = buckets per lane of the next grab
    uint32_t grab = 1, base = 0, left = 0;
    for (;;) {
        if (!left) {
            uint32_t b0 = 0;
            if (lane == 0) b0 = atomicAdd(queue, 64u * grab);
            base = (uint32_t)__builtin_amdgcn_readfirstlane((int)b0);
            left = grab;
        }
        if (base >= nb) break;
        const uint32_t tq = base + lane;
        const bool first = left == grab;
        base += 64u; left--;
        if (tq >= nb) continue;
        const uint2 oc = order[tq];
        if (first && (uint32_t)__builtin_amdgcn_readfirstlane((int)oc.y) == 1u) grab = GF_GRAB_EG;   // single-packet tail
        for (uint32_t k = 0; k < oc.y; k++) {
            const uint32_t i = perm[oc.x + k];
            const EgRec r = erec[i];
            gf_rec rr;
            if (r.st) continue;                         // final in the front (its pass-2 record is written)
            gf_egress_out o{};
            o.stage = GF_STAGE_FROM_LXC;
            o.slave = r.slave; o.rev_nat = r.rev_nat; o.eg_flags = r.eflags;
            uint32_t ifx = 0, lxc = 0, ab = 24 + 34 + 32;
            uint8_t *g = E.snap + (size_t)i * E.stride;
            constexpr bool v6 = FAM == 6;
            int ret;
            PktHdr h2;                                  // the delivered header, re-parsed (local deliveries)
            if constexpr (v6) {                         // the frame in HBM
                Row w{g, E.stride < r.len ? E.stride : r.len};
                ret = eg_ct_part6<PCT>(E, r, i, w, o, ifx, lxc, &added, ab);
                if (ret == ND_TAILCALL) parse_row(w.p, w.cap, r.len, h2);
            } else {                                    // the LDS copy of the header bytes
                eg_copy(row, g, K);
                Row w{row, K < r.len ? K : r.len};
                ret = eg_ct_part<PCT>(E, r, i, w, o, ifx, lxc, &added, seq, rlog, ab);
                if (ret == ND_TAILCALL) parse_row(w.p, w.cap, r.len, h2);
                eg_copy(g, row, K);
            }
            o.ct_ret = o.eg_ct_ret;
            if constexpr (PCT) {
                if (added && !(E.strict & (FAM == 6 ? 2u : 1u))) {
                    const gf_lxc_dev *c = E.cfgs + (r.ep - 1);
                    atomicAdd(gload<uint32_t *>(FAM == 6 ? &c->ct6.count : &c->ct4.count), (uint32_t)added);
                }
                added = 0;
            }
            if (ret == ND_ICMP6_TE) {                   // ipv6_l3 -> icmp6_send_time_exceeded: the reply goes out
                ret = TC_REDIRECT; ifx = 0;
                o.eg_flags |= GF_EG_F_ICMP6_TE;
            }
            if (ret == ND_TAILCALL) {                   // handle_policy of the destination, next pass
                o.stage = GF_STAGE_POLICY; o.lxc_id = (uint16_t)lxc; o.ct_ret = 0;
                const gf_lxc_dev *c = E.cfgs + (r.ep - 1);
                uint32_t kk = pack_rec(i, h2.et, r.len, h2.sa, h2.da, h2.w0, h2.w3, h2.l4, h2.proto,
                                       gload<uint32_t>(&c->seclabel), ifx, E.slot_of[lxc & 0xffffu], 0, false, true,
                                       h2.s6, h2.d6, rr, E.K);
                if (E.conn) {                           // the delivery's connection (handle_policy's CT tuple)
                    E.key2P[i] = kk;
                    if (h2.et == 0x0800 && r.len >= 34) {
                        const bool tu = h2.proto == 6 || h2.proto == 17;
                        kk = gf_key_live(gf_conn_hash4(h2.sa, tu ? (h2.w0 & 0xffffu) : 0u, h2.da, tu ? (h2.w0 >> 16) : 0u,
                                                       h2.proto), E.K);
                    }
                }
                key2[i] = kk;
                rec2[i] = rr;
                if constexpr (v6) {
                    reinterpret_cast<uint4 *>(E.s6out)[2 * (size_t)i] = make_uint4(h2.s6[0], h2.s6[1], h2.s6[2], h2.s6[3]);
                    reinterpret_cast<uint4 *>(E.d6out)[2 * (size_t)i] = make_uint4(h2.d6[0], h2.d6[1], h2.d6[2], h2.d6[3]);
                    atomicAdd(E.ctlog_n + 1, 1u);       // the ingress pass needs its IPv6 kernel
                }
                if (stats) { ls[2] += ab; if (ls[2] >= 0xf0000000u) fold(); }
            } else {
                if (ret < 0 || ret == TC_SHOT) {
                    o.action = TC_SHOT; o.reason = (uint8_t)(-ret);
                    o.eg_flags &= (GF_EG_F_CREATED | GF_EG_F_DELETED | GF_EG_F_LB | GF_EG_F_LOOPBACK | GF_EG_F_PORTMAP |
                                   GF_EG_F_REVNAT | GF_EG_F_IPV6);
                    o.proxy_port = 0; o.tunnel_ip = 0;
                } else {
                    o.action = (uint8_t)ret;
                    o.ifindex_lo = (uint16_t)ifx;
                }
                if (stats) {
                    st.add(o.reason); st.add(256 + o.action);
                    ls[0] += 1; ls[1] += r.len; ls[2] += ab;
                    if (ls[1] >= 0xf0000000u || ls[2] >= 0xf0000000u) fold();
                }
            }
            out[i] = o;
        }
    }
    if (!(E.strict & (FAM == 6 ? 2u : 1u))) {       // strict maps counted each insert inline
        if (added) atomicAdd(&sadd, (uint32_t)added);
        __syncthreads();
        if (threadIdx.x == 0 && sadd && ct_count) atomicAdd(ct_count, sadd);
    }
    if (stats) { fold(); st.flush(stats); }
}

// The deferred service entries of a launch, in batch order (k_px_apply's rule):
// sorted by (key hash, packet index), an entry is applied only if no later
// entry of the batch has the same key.
// The logged ct_create entries (service entries of the from-container pass,
// related entries of connection groups), applied last-writer-wins per CT key:
// k_ctlog_max enters every entry into a scratch open-addressing set keyed by the
// logged tuple.  A slot is one u64: (1 + the highest order entered for its key)
// << 32 | that entry's index, 0 = empty; the key of a slot is its current entry's
// (every entry ever held by a slot has the slot's key).  A key's first entry
// claims a slot with one CAS, a later one raises it with atomicMax (the order in
// the high half), so a key logged once — most of them — costs one atomic.
// k_ctlog_apply walks the set's slots and upserts each key's winning entry.  Log
// entry: [0] order, [1..4] the 14-B key, [5..16] the 48-B value.
template <bool PCT = false>
__device__ __forceinline__ bool ctlog_same(const uint32_t *a, const uint32_t *b) {
    if (PCT && (a[18] != b[18] || a[19] != b[19])) return false;   // per-endpoint maps: the same map too
    return a[1] == b[1] && a[2] == b[2] && a[3] == b[3] && (a[4] & 0xffffu) == (b[4] & 0xffffu);
}
// The set is sized for the entries actually logged (<= 1/2 load; the count is on
// the device) inside an allocation made for the call's upper bound: both kernels
// derive the mask from the count themselves, and k_ctlog_apply leaves every slot it
// walks zero again — the set is all zero between applies (zeroed once when it is
// allocated), so no launch of its own clears it.
__device__ __forceinline__ uint32_t ctlog_mask(uint32_t n, uint32_t cap_mask) {
    const uint64_t want = 2ull * n;
    uint32_t t = 1023u;
    while ((uint64_t)t + 1 < want && t < cap_mask) t = t * 2 + 1;
    return t < cap_mask ? t : cap_mask;
}
template <bool PCT = false>
__global__ __launch_bounds__(BLOCK) void k_ctlog_max(const uint32_t *lg, const uint32_t *n_, unsigned long long *tab,
                                                     uint32_t cap_mask) {
    const uint32_t n = *n_, tmask = ctlog_mask(n, cap_mask);
    const uint32_t j = blockIdx.x * BLOCK + threadIdx.x;
    if (j >= n) return;
    const uint32_t *e = lg + (size_t)GF_CTLOG_WORDS * j;
    const unsigned long long want = ((unsigned long long)(e[0] + 1u) << 32) | j;
    uint32_t h0 = key_hash<14, GF_HASH_CT>(e + 1);
    if constexpr (PCT) h0 ^= gf_hash_words(e + 18, 2, 8);   // (the same tuple in two maps: two keys)
    for (uint32_t p = h0 & tmask;; p = (p + 1) & tmask) {
        // plain read first: a stale 0 only makes the CAS fail, a stale value only
        // costs the atomicMax it would have skipped
        unsigned long long cur = tab[p];
        if (cur == 0ull) {
            cur = atomicCAS(&tab[p], 0ull, want);
            if (cur == 0ull) return;                    // claimed for this key
        }
        if (ctlog_same<PCT>(lg + (size_t)GF_CTLOG_WORDS * (uint32_t)cur, e)) {
            if (cur < want) atomicMax(&tab[p], want);
            return;
        }
    }
}
// PCT: each entry into its program's own map (cfgs; ct, ct_count unused).
template <bool PCT = false>
__global__ __launch_bounds__(BLOCK) void k_ctlog_apply(const uint32_t *lg, const uint32_t *n_, unsigned long long *tab,
                                                       uint32_t cap_mask, gf_htab_desc ct, uint32_t *ct_count,
                                                       const gf_lxc_dev *cfgs = nullptr) {
    const uint32_t tmask = ctlog_mask(*n_, cap_mask);
    int added = 0;
    for (uint64_t p = blockIdx.x * (uint64_t)BLOCK + threadIdx.x; p <= tmask; p += (uint64_t)gridDim.x * BLOCK) {
        const unsigned long long t = tab[p];
        if (t == 0ull) continue;                        // an empty slot
        tab[p] = 0ull;                                  // the set is clean for its next use
        const uint32_t *e = lg + (size_t)GF_CTLOG_WORDS * (uint32_t)t;   // the key's last entry in order
        if constexpr (PCT) {
            const gf_htab_desc d = gload<gf_htab_desc>(&cfgs[e[17] - 1].ct4);
            int a = 0;
            ht_upsert<14, 12, GF_HASH_CT, GF_CT4_U>(d, e + 1, e + 5, false, &a);
            if (a) atomicAdd(d.count, (uint32_t)a);
        } else {
            ht_upsert<14, 12, GF_HASH_CT, GF_CT4_U>(ct, e + 1, e + 5, false, &added);
        }
    }
    if (!ct_count || !__any(added != 0)) return;
    uint32_t tot = (uint32_t)added;                     // one count add per wave
    for (int d = 32; d >= 1; d >>= 1) tot += (uint32_t)__shfl_xor((int)tot, d);
    if ((threadIdx.x & 63u) == 0u) atomicAdd(ct_count, tot);
}

// The winners of a connection-group run's related-entry set (RelSet), written after
// the run: each claimed slot's one or two keys get the value their last writer's
// ct_create4 builds (conntrack.h:563-577) — order 2i: packet i's from-container create
// (the sender's SECLABEL and tx counters, bpf_lxc.c:534), 2i + 1: its delivery's
// handle_policy create (src_sec_id the source identity, rx counters, bpf_lxc.c:941) —
// and the slot is left zero for the next run.
__global__ __launch_bounds__(BLOCK) void k_rset_apply(RelSet R, const EgRec *erec, const gf_rec *rec,
                                                      const gf_lxc_dev *cfgs, gf_htab_desc ct, uint32_t *ct_count,
                                                      uint32_t now) {
    const uint32_t n = *R.list_n;
    int added = 0;
    for (uint32_t j = blockIdx.x * BLOCK + threadIdx.x; j < n; j += gridDim.x * BLOCK) {
        const uint32_t p = R.list[j];
        const uint4 sl = *reinterpret_cast<const uint4 *>(R.slot + 2ull * p);
        const unsigned long long k = p == R.mask + 1u ? 0ull : ((unsigned long long)sl.y << 32) | sl.x;
        for (uint32_t side = 0; side < 2; side++) {
            const uint32_t w = side ? sl.w : sl.z;
            if (!w) continue;
            const uint32_t o = w - 1u, i = o >> 1;
            const uint32_t it[4] = {(uint32_t)(k >> 32), (uint32_t)k, 0u, 1u | ((2u | side) << 8)};
            uint32_t v[12] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
            if (o & 1u) {                               // handle_policy (rev_nat 0 on ingress)
                const gf_rec r = rec[i];
                const uint32_t fl = r.proto == 6 ? 0u : F_SEEN_NON_SYN;
                v[0] = now + ((fl & F_SEEN_NON_SYN) ? 43200u : 300u);
                v[1] = fl | F_SEEN_NON_SYN;
                v[2] = 1u; v[3] = r.len; v[11] = r.src_identity;
            } else {                                    // from-container
                const EgRec r = erec[i];
                uint32_t efl = r.nh == 6 ? 0u : F_SEEN_NON_SYN;
                if (r.eflags & GF_EG_F_LOOPBACK) efl |= F_LB_LOOPBACK;
                v[0] = now + ((efl & F_SEEN_NON_SYN) ? 43200u : 300u);
                v[1] = efl | F_SEEN_NON_SYN | ((uint32_t)r.rev_nat << 16);
                v[6] = 1u; v[8] = r.len; v[11] = gload<uint32_t>(&cfgs[r.ep - 1].seclabel);
            }
            ht_upsert<14, 12, GF_HASH_CT, GF_CT4_U>(ct, it, v, false, &added);
        }
        *reinterpret_cast<uint4 *>(R.slot + 2ull * p) = make_uint4(0u, 0u, 0u, 0u);
    }
    if (!ct_count || !__any(added != 0)) return;
    uint32_t tot = (uint32_t)added;                     // one count add per wave
    for (int d = 32; d >= 1; d >>= 1) tot += (uint32_t)__shfl_xor((int)tot, d);
    if ((threadIdx.x & 63u) == 0u) atomicAdd(ct_count, tot);
}

// ---- host: the launch profiler, call contexts (CallCtx), check_cols, the call order (CallOrder) ----
#include "gf_host_ctx.h"

// ---- host: program loads and the column calls: gf_parse_frames, gf_xdp_*, gf_lb_*, gf_lxc_prog_load ----
#include "gf_host_programs.h"

// handle_policy over a batch (caller holds prog_lock and the maps' locks, and checked the columns).
// skip (DEVICE, may be null): packets a pipeline ended before the tail call.
// Trace notifications of a call: per-packet marks and captures (GF_TR_*),
// allocated and the marks cleared by the caller before its first kernel.
struct TraceWs { DevBuf mark, px, in; };
static TraceWs &trace_ws() { static const char tag = 0; return cur_ctx().get<TraceWs>(&tag); }
// Who runs a handle_policy pass (the values are EvSrc::kind's).
enum class PassKind : uint32_t {
    Plain = 0,                     // gf_policy_ingress_classify(_batches): packet columns in, gf_ingress_out out
    Frames = 1,                    // a frame entry point (pipeline, from-overlay, from-host): its front packs
    Egress = 2,                    // the local deliveries of gf_lxc_egress_classify
};
// Fills the records and bucket keys itself (a fused front) instead of k_ing_pack.
using PackFn = std::function<int(const uint16_t *slot_of, gf_rec *rec, uint32_t *keys)>;
// One handle_policy pass (ingress_run).  Default-constructed: the plain gf_policy_ingress_classify call.
struct PolicyPass {
    PassKind kind = PassKind::Plain;
    gf_ingress_out *out = nullptr; // plain: the verdict records, or
    uint8_t *pout = nullptr;       // frames / egress: the 24-byte pipeline records to complete
    PackFn pack;                   // may be empty: k_ing_pack over the columns
    const uint32_t *ev_len = nullptr;  // the notifications' lengths (null: the len column), frames and their stride;
    const uint8_t *ev_snap = nullptr;  // ev_stride is wsnap's stride too
    uint32_t ev_stride = 0;
    uint8_t *wsnap = nullptr;      // frames handle_policy writes (a proxy redirect's MAC stores), or null
    bool lru = true;               // the LRU stand-in after the pass
    bool px_keep = false;          // continue the cilium_proxy log the same call's earlier pass began (px_log_begin)
    bool prepared = false;         // pack + schedule already built in ws() (ingress_prepare)
    uint32_t *rlog = nullptr, *rlog_n = nullptr;   // egress connection groups: the related-entry log (null: written inline)
    const uint32_t *rlog_off = nullptr;            // device word: the run fell back to pair groups (the log is not used)
    RelSet rs{};                   // the related entries' set (rlog then only marks it in use)
    bool on = false;               // frames / egress: this call traces (a ring is set and a program / the netdev traces)
    uint32_t nd_trace = 0, nd_ifindex = 0;   // pipeline / overlay: 0, or the front's observation point | its final
                                   // stage << 8 (EvSrc::nd_trace); skb->ingress_ifindex
    const uint8_t *orig = nullptr;     // egress: the frames as sent
    const uint16_t *lxc_id = nullptr;  // egress: the senders
    bool keep_flags = false;       // from-host: the front's record holds a flag gf_rec.cls does not carry
                                   // (GF_PIPE_F_REV_PROXY), so handle_policy completes it by read-modify-write
    const uint32_t *hmark = nullptr;   // from-host: the mark column (EvSrc::hmark)
};
static bool array_traces(const std::shared_ptr<PolicyArray> &a) {
    if (!a) return false;
    for (auto &kv : a->slots)
        if (kv.second->cfg.flags & GF_LXC_F_TRACE_NOTIFY) return true;
    return false;
}
// Programs without conntrack (GF_LXC_F_NO_CONNTRACK) in an array: 0 none, 1 some, 2 every one.
// Kept on the array by gf_policy_array_update (a program's flags never change).
static int array_noct(const std::shared_ptr<PolicyArray> &a) { return a->noct; }
// Debug notifications of a plain ingress call: the per-packet log column (DbgLog), cleared.
struct DbgWs { DevBuf log; };
static DbgWs &dbg_ws() { static const char tag = 0; return cur_ctx().get<DbgWs>(&tag); }
// (32 B per packet of the batch, kept for the context's later calls: a call that cannot get it
// fails with -ENOMEM although the same call without a debug program would run; gpuflow.h says so)
static int dbg_prepare(uint32_t n, hipStream_t s) {
    DbgWs &d = dbg_ws();
    const size_t want = (size_t)n * 32;
    int r;
    if (d.log.bytes < want && (r = d.log.ensure(want))) return r;
    return hip_ok(hipMemsetAsync(d.log.p, 0, want, s), "debug log");
}

static int trace_prepare(uint32_t n, bool with_in, hipStream_t s) {
    TraceWs &t = trace_ws();
    auto grow = [](DevBuf &d, size_t want) -> int { return d.bytes >= want ? 0 : d.ensure(want); };
    int r;
    if ((r = grow(t.mark, (size_t)n + 16)) || (r = grow(t.px, (size_t)n * GF_TRACE_PAYLOAD_LEN)) ||
        (with_in && (r = grow(t.in, (size_t)n * GF_TRACE_PAYLOAD_LEN))))
        return r;
    return hip_ok(hipMemsetAsync(t.mark.p, 0, n, s), "trace marks");
}

// Drop (and trace) notifications of one classify call (no-op without an event ring).
static int emit_drop_events(EvSrc E, hipStream_t s, bool dbg = false) {
    gf_event_ring R = event_ring();
    if (!R.records || !R.count || !R.capacity || E.n == 0) return 0;
    struct EvWs { DevBuf blk, boff, tmp; };
    static const char tag = 0;
    EvWs &ew = cur_ctx().get<EvWs>(&tag);
    DevBuf &blk = ew.blk, &boff = ew.boff, &tmp = ew.tmp;
    const uint32_t nb = (E.n + BLOCK - 1) / BLOCK;
    auto grow = [](DevBuf &d, size_t want) -> int { return d.bytes >= want ? 0 : d.ensure(want); };
    int r;
    if ((r = grow(blk, (size_t)nb * 4)) || (r = grow(boff, (size_t)nb * 4))) return r;
    size_t tb = 0;
    (void)rocprim::exclusive_scan(nullptr, tb, (uint32_t *)blk.p, (uint32_t *)boff.p, 0u, nb, rocprim::plus<uint32_t>(), s);
    if ((r = grow(tmp, tb + 256))) return r;
    ProfScope ps("k_drop_events", s);
    if (dbg) hipLaunchKernelGGL(k_ev_count_dbg, dim3(nb), dim3(BLOCK), 0, s, E, (uint32_t *)blk.p);
    else hipLaunchKernelGGL(k_ev_count, dim3(nb), dim3(BLOCK), 0, s, E, (uint32_t *)blk.p);
    tb = tmp.bytes;
    if (hip_ok(rocprim::exclusive_scan(tmp.p, tb, (uint32_t *)blk.p, (uint32_t *)boff.p, 0u, nb,
                                       rocprim::plus<uint32_t>(), s), "event scan"))
        return -EIO;
    if (dbg) hipLaunchKernelGGL(k_ev_write_dbg, dim3(nb), dim3(BLOCK), 0, s, E, (const uint32_t *)boff.p, R);
    else hipLaunchKernelGGL(k_ev_write, dim3(nb), dim3(BLOCK), 0, s, E, (const uint32_t *)boff.p, R);
    hipLaunchKernelGGL(k_ev_commit, dim3(1), dim3(1), 0, s, (const uint32_t *)boff.p, (const uint32_t *)blk.p, nb, R);
    return hip_ok(hipGetLastError(), "k_drop_events");
}

// Per-batch workspace of the flow-group schedule (records, keys, sort, runs, order).
static int ws_grow(uint32_t n) {
    Workspace &w = ws();
    auto grow = [](DevBuf &b, size_t want) -> int { return b.bytes >= want ? 0 : b.ensure(want); };
    int r;
    if ((r = grow(w.rec, (size_t)n * sizeof(gf_rec))) || (r = grow(w.keys, (size_t)n * 4)) ||
        (r = grow(w.skeys, (size_t)n * 4)) || (r = grow(w.perm, (size_t)n * 4 + 16)) ||
        (r = grow(w.off, (size_t)n * 4)) || (r = grow(w.order, (size_t)n * 8)) ||
        (r = grow(w.sched, GF_SCHED_WORDS * 4)))
        return r;
    return 0;
}

// The flow-group schedule of ws().keys[0..n): stable radix sort of (bucket key of
// gf_key_for(n) bits, index), the start of every run of equal hashes (one bucket per run: a
// select of the positions whose key differs from the one before), then the
// longest-first bucket order per family, built on the device (no host round
// trip): ws().perm / order / sched.
// GF_SORT_RADIX (gf_common.h): digit bits of the onesweep passes; 8 is rocPRIM's gfx950 default
#ifndef GF_SORT_IPT
#define GF_SORT_IPT 16
#endif
#if GF_SORT_RADIX == 8 && GF_SORT_IPT == 16
using GfSortCfg = rocprim::default_config;
#else
using GfSortCfg = rocprim::radix_sort_config<
    rocprim::default_config, rocprim::default_config,
    rocprim::radix_sort_onesweep_config<rocprim::kernel_config<1024, GF_SORT_IPT>, rocprim::kernel_config<1024, GF_SORT_IPT>,
                                        GF_SORT_RADIX, rocprim::block_radix_rank_algorithm::match>>;
#endif
// The schedule's sort of (key, index): GfSortCfg's digits below 32 key bits; a 32-bit
// key takes rocPRIM's default config (four 8-bit passes are cheaper than 9/9/9/5).
static hipError_t sort_keys(void *tmp, size_t &bytes, const uint32_t *keys, uint32_t *skeys, uint32_t *perm, uint32_t n,
                            uint32_t bits, hipStream_t s) {
    const rocprim::counting_iterator<uint32_t> idx(0u);
    if (bits == 32 && !GF_KEY_BITS)
        return rocprim::radix_sort_pairs<rocprim::default_config>(tmp, bytes, keys, skeys, idx, perm, n, 0, bits, s);
    return rocprim::radix_sort_pairs<GfSortCfg>(tmp, bytes, keys, skeys, idx, perm, n, 0, bits, s);
}
// Run starts of the sorted keys in three passes over GF_RUN_ITEMS-key tiles:
// count the starts per tile, scan the tile counts (one block), write each
// tile's starts at its offset in position order (wave ballots + LDS scan).
__device__ __forceinline__ bool run_start(const uint32_t *k, uint32_t j) { return j == 0 || k[j] != k[j - 1]; }
// zero: n words to clear on the way (the single-bucket words of an egress schedule,
// k_single_mark: one launch fewer than a fill of their own), or null
__global__ __launch_bounds__(BLOCK) void k_run_count(uint32_t n, const uint32_t *skeys, uint32_t *tcnt,
                                                     uint32_t *zero = nullptr) {
    __shared__ uint32_t wc[BLOCK / 64];
    const uint32_t b0 = blockIdx.x * GF_RUN_ITEMS, lane = threadIdx.x & 63u;
    uint32_t c = 0;
    for (uint32_t k = 0; k < GF_RUN_ITEMS / BLOCK; k++) {
        const uint32_t j = b0 + k * BLOCK + threadIdx.x;
        c += (uint32_t)__popcll(__ballot(j < n && run_start(skeys, j)));
        if (zero && j < n) zero[j] = 0u;
    }
    if (lane == 0) wc[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t = 0;
        for (uint32_t w = 0; w < BLOCK / 64; w++) t += wc[w];
        tcnt[blockIdx.x] = t;
    }
}
// zero / nzero: words to clear on the way (the schedule's bucket histogram: one
// launch fewer than a fill of its own)
__global__ __launch_bounds__(1024) void k_run_scan(uint32_t nt, uint32_t *tcnt, uint32_t *nruns, uint32_t *zero = nullptr,
                                                   uint32_t nzero = 0) {
    __shared__ uint32_t part[1024];
    __shared__ uint32_t carry;
    for (uint32_t k = threadIdx.x; k < nzero; k += 1024) zero[k] = 0;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (uint32_t c0 = 0; c0 < nt; c0 += 1024) {         // exclusive scan in place, 1024 tiles at a time
        const uint32_t t = c0 + threadIdx.x;
        const uint32_t v = t < nt ? tcnt[t] : 0u;
        part[threadIdx.x] = v;
        __syncthreads();
        for (uint32_t o = 1; o < 1024; o <<= 1) {
            const uint32_t x = threadIdx.x >= o ? part[threadIdx.x - o] : 0u;
            __syncthreads();
            part[threadIdx.x] += x;
            __syncthreads();
        }
        if (t < nt) tcnt[t] = carry + part[threadIdx.x] - v;
        __syncthreads();
        if (threadIdx.x == 1023) carry += part[1023];
        __syncthreads();
    }
    if (threadIdx.x == 0) *nruns = carry;
}
__global__ __launch_bounds__(BLOCK) void k_run_write(uint32_t n, const uint32_t *skeys, const uint32_t *toff,
                                                     uint32_t *off) {
    __shared__ uint32_t wc[BLOCK / 64];
    const uint32_t b0 = blockIdx.x * GF_RUN_ITEMS, lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    uint32_t base = toff[blockIdx.x];
    for (uint32_t k = 0; k < GF_RUN_ITEMS / BLOCK; k++) {
        const uint32_t j = b0 + k * BLOCK + threadIdx.x;
        const bool f = j < n && run_start(skeys, j);
        const uint64_t m = __ballot(f);
        if (lane == 0) wc[wv] = (uint32_t)__popcll(m);
        __syncthreads();
        uint32_t before = 0, all = 0;
        for (uint32_t w = 0; w < BLOCK / 64; w++) { before += w < wv ? wc[w] : 0u; all += wc[w]; }
        if (f) off[base + before + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = j;
        base += all;
        __syncthreads();
    }
}
// single: single-packet buckets in packet-index order (the egress passes).
// wide: the keys came from a frame front (gf_key_for(n, true)).
static int schedule_groups(uint32_t n, hipStream_t s, bool single = false, bool wide = false) {
    Workspace &w = ws();
    const gf_key_cfg K = gf_key_for(n, wide);           // the width the keys were built with: the same rule, the same n
    auto grow = [](DevBuf &b, size_t want) -> int { return b.bytes >= want ? 0 : b.ensure(want); };
    int r;
    uint32_t *d_sched = (uint32_t *)w.sched.p, *d_nruns = GF_SCHED_NRUNS(d_sched);
    size_t sort_bytes = 0;
    (void)sort_keys(nullptr, sort_bytes, (const uint32_t *)w.keys.p, (uint32_t *)w.skeys.p, (uint32_t *)w.perm.p, n,
                    K.bits, s);
    const uint32_t nt = (n + GF_RUN_ITEMS - 1) / GF_RUN_ITEMS;
    if ((r = grow(w.tmp, sort_bytes + 256)) || (r = grow(w.tcnt, (size_t)nt * 4 + 16))) return r;
    if (single && ((r = grow(w.sb, (size_t)n * 4)) || (r = grow(w.st0, (size_t)nt * 4 + 16)) ||
                   (r = grow(w.st1, (size_t)nt * 4 + 16))))
        return r;
    size_t tb = w.tmp.bytes;
    {
        ProfScope ps("rocprim_radix_sort", s);
        if (hip_ok(sort_keys(w.tmp.p, tb, (const uint32_t *)w.keys.p, (uint32_t *)w.skeys.p, (uint32_t *)w.perm.p, n,
                             K.bits, s), "radix_sort_pairs"))
            return -EIO;
    }
    {
        ProfScope ps("bucket_runs", s);
        if (nt) hipLaunchKernelGGL(k_run_count, dim3(nt), dim3(BLOCK), 0, s, n, (const uint32_t *)w.skeys.p,
                                   (uint32_t *)w.tcnt.p, single ? (uint32_t *)w.sb.p : nullptr);
        hipLaunchKernelGGL(k_run_scan, dim3(1), dim3(1024), 0, s, nt, (uint32_t *)w.tcnt.p, d_nruns,
                           GF_SCHED_HIST(d_sched), GF_SCHED_HBYTES / 4u);   // (+ the bucket histogram cleared)
        if (nt) hipLaunchKernelGGL(k_run_write, dim3(nt), dim3(BLOCK), 0, s, n, (const uint32_t *)w.skeys.p,
                                   (const uint32_t *)w.tcnt.p, (uint32_t *)w.off.p);
        if ((r = hip_ok(hipGetLastError(), "run starts"))) return r;
    }
    {
        ProfScope ps("k_bucket_sched", s);
        static const bool lds_ok = [] {                  // the bins are > 64 KB of dynamic LDS
            return hipFuncSetAttribute((const void *)k_bucket_hist, hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)GF_SCHED_HBYTES) == hipSuccess &&
                   hipFuncSetAttribute((const void *)k_bucket_order, hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)GF_SCHED_HBYTES) == hipSuccess;
        }();
        if (!lds_ok) return hip_ok(hipErrorInvalidValue, "k_bucket_sched LDS");
        uint32_t g = (n + GF_SCHED_ITEMS - 1) / GF_SCHED_ITEMS;
        hipLaunchKernelGGL(k_bucket_hist, dim3(g), dim3(BLOCK), GF_SCHED_HBYTES, s, n, (const uint32_t *)w.off.p,
                           (const uint32_t *)w.skeys.p, (const gf_rec *)nullptr, (const uint32_t *)w.perm.p, d_sched, K);
        hipLaunchKernelGGL(k_bucket_base, dim3(1), dim3(GF_LCAP), 0, s, d_sched);
        hipLaunchKernelGGL(k_bucket_order, dim3(g), dim3(BLOCK), GF_SCHED_HBYTES, s, n, (const uint32_t *)w.off.p,
                           (const uint32_t *)w.skeys.p, (const gf_rec *)nullptr, (const uint32_t *)w.perm.p, d_sched, (uint2 *)w.order.p,
                           single ? 1u : 0u, K);
        if (single) {                                   // (the words were cleared by k_run_count)
            hipLaunchKernelGGL(k_single_mark, dim3(std::min<uint32_t>((n + BLOCK - 1) / BLOCK, 8192u)), dim3(BLOCK), 0, s, n,
                               (const uint32_t *)w.off.p, (const uint32_t *)w.skeys.p, (const uint32_t *)w.perm.p,
                               (const uint32_t *)d_sched, (uint32_t *)w.sb.p, K);
            hipLaunchKernelGGL(k_single_count, dim3(nt), dim3(BLOCK), 0, s, n, (const uint32_t *)w.sb.p,
                               (uint32_t *)w.st0.p, (uint32_t *)w.st1.p);
            hipLaunchKernelGGL(k_run_scan, dim3(1), dim3(1024), 0, s, nt, (uint32_t *)w.st0.p, (uint32_t *)w.st0.p + nt,
                               nullptr, 0u);
            hipLaunchKernelGGL(k_run_scan, dim3(1), dim3(1024), 0, s, nt, (uint32_t *)w.st1.p, (uint32_t *)w.st1.p + nt,
                               nullptr, 0u);
            hipLaunchKernelGGL(k_single_write, dim3(nt), dim3(BLOCK), 0, s, n, (const uint32_t *)w.sb.p,
                               (const uint32_t *)w.st0.p, (const uint32_t *)w.st1.p, (const uint32_t *)d_sched,
                               (uint2 *)w.order.p);
        }
    }
    return hip_ok(hipGetLastError(), "k_bucket_sched");
}

// cilium_proxy{4,6} update log of one launch (pol_redirect) and its in-order
// apply after the launch (see k_px_apply).
struct PxWs {
    DevBuf plog, plog_n, pkey, pkey2, pval, pperm, ptmp;
    bool live = false;         // a log was begun in this call (its count is valid)
};
static PxWs &px_ws() { static const char tag = 0; return cur_ctx().get<PxWs>(&tag); }
// keep: continue the log the from-container pass of the same egress call wrote
// (each packet logs at most one update: an egress redirect is never delivered).
// Without proxy maps the updates are no-ops that succeed (the reference's maps
// always exist), but a redirect still gets the MAC stores that follow it in
// ipv{4,6}_policy when the call writes frames: the log is kept for those.
static int px_log_begin(uint32_t n, hipStream_t s, IngCtx &X, bool keep = false) {
    auto px4 = proxy_map(4), px6 = proxy_map(6);
    X.plog = nullptr; X.plog_n = nullptr;
    PxWs &w = px_ws();
    if (!px4 && !px6 && !X.snap && !(keep && w.live)) { w.live = keep && w.live; return 0; }
    int r;
    auto grow = [](DevBuf &b, size_t want) -> int { return b.bytes >= want ? 0 : b.ensure(want); };
    if ((r = grow(w.plog, (size_t)n * 64)) || (r = grow(w.plog_n, 4))) return r;
    if ((!keep || !w.live) && hip_ok(hipMemsetAsync(w.plog_n.p, 0, 4, s), "plog_n")) return -EIO;
    w.live = true;
    for (auto &m : {px4, px6})
        if (m && (r = push_map(m, s))) return r;
    X.plog = (uint32_t *)w.plog.p; X.plog_n = (uint32_t *)w.plog_n.p;
    return 0;
}
// recs: the launch's verdict records (24-B pipeline/egress layout when wide, else gf_ingress_out)
static int px_log_apply(const IngCtx &X, hipStream_t s, uint8_t *wsnap, const uint32_t *len, uint32_t stride,
                        uint8_t *recs, bool wide, uint32_t n) {
    if (!X.plog) return 0;
    px_ws().live = false;
    auto px4 = proxy_map(4), px6 = proxy_map(6);
    const gf_node_cfg &node = node_cfg();
    PxWs &w = px_ws();
    int r;
    if (!px4 && !px6) {                               // the MAC stores alone: the count stays on the device
        if (!wsnap) return 0;
        PxDev P{};
        P.snap = wsnap; P.len = len; P.snap_stride = stride;
        memcpy(P.host_mac, node.host_mac, 6); memcpy(P.node_mac, node.node_mac, 6);
        ProfScope ps("k_proxy_apply", s);
        hipLaunchKernelGGL(k_px_macs, dim3(grid_for(n)), dim3(BLOCK), 0, s, (const uint32_t *)X.plog,
                           (const uint32_t *)X.plog_n, P);
        return hip_ok(hipGetLastError(), "k_px_macs");
    }
    uint32_t cnt = 0;
    if (hip_ok(hipMemcpyAsync(&cnt, X.plog_n, 4, hipMemcpyDeviceToHost, s), "plog count") ||
        hip_ok(hipStreamSynchronize(s), "plog sync"))
        return -EIO;
    if (!cnt) return 0;
    PxDev P{};
    bool seq = false;
    for (auto &m : {px4, px6}) {
        if (!m) continue;
        if (m->host_valid) m->dev_count_hi = m->ht.count;
        if (m->dev_count_hi + cnt > m->max_entries) seq = true;
    }
    if (px4) P.d4 = px4->hdesc();
    if (px6) P.d6 = px6->hdesc();
    P.snap = wsnap; P.len = len; P.snap_stride = stride;
    memcpy(P.host_mac, node.host_mac, 6); memcpy(P.node_mac, node.node_mac, 6);
    auto grow = [](DevBuf &b, size_t want) -> int { return b.bytes >= want ? 0 : b.ensure(want); };
    if ((r = grow(w.pkey, (size_t)cnt * 8)) || (r = grow(w.pkey2, (size_t)cnt * 8)) || (r = grow(w.pval, (size_t)cnt * 4)) ||
        (r = grow(w.pperm, (size_t)cnt * 4)))
        return r;
    size_t tb = 0;
    (void)rocprim::radix_sort_pairs(nullptr, tb, (unsigned long long *)w.pkey.p, (unsigned long long *)w.pkey2.p,
                                    (uint32_t *)w.pval.p, (uint32_t *)w.pperm.p, cnt, 0, 64, s);
    if ((r = grow(w.ptmp, tb + 256))) return r;
    ProfScope ps("k_proxy_apply", s);
    const uint32_t g = (cnt + BLOCK - 1) / BLOCK;
    hipLaunchKernelGGL(k_px_keys, dim3(g), dim3(BLOCK), 0, s, (const uint32_t *)w.plog.p, cnt, seq,
                       (unsigned long long *)w.pkey.p, (uint32_t *)w.pval.p);
    tb = w.ptmp.bytes;
    if (hip_ok(rocprim::radix_sort_pairs(w.ptmp.p, tb, (unsigned long long *)w.pkey.p, (unsigned long long *)w.pkey2.p,
                                         (uint32_t *)w.pval.p, (uint32_t *)w.pperm.p, cnt, 0, 64, s), "proxy sort"))
        return -EIO;
    if (seq)
        hipLaunchKernelGGL(k_px_apply_seq, dim3(1), dim3(1), 0, s, (const uint32_t *)w.plog.p, cnt,
                           (const uint32_t *)w.pperm.p, P, recs, wide ? 24u : 8u, wide ? 1u : 0u,
                           (unsigned long long *)stats_sink());
    else
        hipLaunchKernelGGL(k_px_apply, dim3(g), dim3(BLOCK), 0, s, (const uint32_t *)w.plog.p, cnt,
                           (const unsigned long long *)w.pkey2.p, (const uint32_t *)w.pperm.p, P);
    if ((r = hip_ok(hipGetLastError(), "k_proxy_apply"))) return r;
    for (auto &m : {px4, px6}) if (m) { m->device_modified(); m->dev_count_hi += cnt; }
    return 0;
}

// A CT map's launch descriptor: an LRU conntrack map's inserts are limited by its
// slot array (dev_insert_limit), not by max_entries (the eviction pass after the
// call brings the count back).
static gf_htab_desc ct_dev_desc(Map &m) {
    gf_htab_desc d = m.hdesc();
    if (m.type == GF_MAP_TYPE_LRU_HASH) d.max_entries = (uint32_t)std::min<uint64_t>(dev_insert_limit(m), 0xffffffffu);
    return d;
}

// The device program table of a cilium_policy array (every bound map pushed to
// HBM first); uploaded only when it changed (programs, bindings, or a map's
// device storage moved).  progs: the distinct programs, slot k+1 = progs[k].
static int prog_table(const std::shared_ptr<PolicyArray> &a, hipStream_t s,
                      std::vector<std::shared_ptr<ProgLxc>> &progs) {
    int r;
    std::map<ProgLxc *, uint32_t> index;
    std::vector<uint16_t> slot_of(65536, 0);
    for (auto &kv : a->slots) {
        auto &p = kv.second;
        auto it = index.find(p.get());
        if (it == index.end()) {
            if (progs.size() >= 65535) return -E2BIG;
            it = index.emplace(p.get(), (uint32_t)progs.size()).first;
            progs.push_back(p);
        }
        slot_of[kv.first] = (uint16_t)(it->second + 1);
    }
    std::vector<gf_lxc_dev> cfgs(progs.size());
    for (size_t k = 0; k < progs.size(); k++) {
        auto &p = progs[k];
        for (auto m : {p->policy, p->ct4, p->ct6, p->cidr4, p->cidr6, p->revnat4, p->revnat6, p->lb4, p->ipcache,
                       p->cidr4e, p->lb6, p->cidr6e})
            if ((r = push_map(m, s))) return r;
        gf_lxc_dev &d = cfgs[k];
        memset(&d, 0, sizeof d);
        d.flags = p->cfg.flags; d.lxc_id = p->cfg.lxc_id; d.seclabel = p->cfg.seclabel;
        d.n_l4 = p->cfg.n_l4_ingress;
        for (uint32_t j = 0; j < d.n_l4; j++) {
            d.l4[j].port = p->cfg.l4_ingress[j].port; d.l4[j].proxy = p->cfg.l4_ingress[j].proxy;
            d.l4[j].nexthdr = p->cfg.l4_ingress[j].nexthdr;
        }
        if (p->policy) d.policy = p->policy->hdesc();
        if (p->ct4) { d.ct4 = ct_dev_desc(*p->ct4); d.flags |= GF_LXC_DEV_HAS_CT4; }
        if (p->ct6) { d.ct6 = ct_dev_desc(*p->ct6); d.flags |= GF_LXC_DEV_HAS_CT6; }
        if (p->cidr4) d.cidr4 = p->cidr4->tdesc();
        if (p->cidr6) d.cidr6 = p->cidr6->tdesc();
        if (p->revnat4) d.revnat4 = p->revnat4->hdesc();
        if (p->revnat6) d.revnat6 = p->revnat6->hdesc();
        memcpy(d.lxc_mac, p->cfg.lxc_mac, 6);
        memcpy(d.node_mac, p->cfg.node_mac, 6);
        d.lxc_ipv4 = p->cfg.lxc_ipv4;
        d.n_portmap = p->cfg.n_portmap;
        for (uint32_t j = 0; j < d.n_portmap; j++)
            d.portmap[j] = p->cfg.portmap[j].from | ((uint32_t)p->cfg.portmap[j].to << 16);
        d.n_l4e = p->cfg.n_l4_egress;
        for (uint32_t j = 0; j < d.n_l4e; j++) {
            d.l4e[j].port = p->cfg.l4_egress[j].port; d.l4e[j].proxy = p->cfg.l4_egress[j].proxy;
            d.l4e[j].nexthdr = p->cfg.l4_egress[j].nexthdr;
        }
        if (p->lb4) d.lb4 = p->lb4->hdesc();
        if (p->ipcache) d.ipcache = p->ipcache->hdesc();
        if (p->cidr4e) d.cidr4e = p->cidr4e->tdesc();
        memcpy(d.lxc_ip6, p->cfg.lxc_ip6, 16);
        if (p->lb6) d.lb6 = p->lb6->hdesc();
        if (p->cidr6e) d.cidr6e = p->cidr6e->tdesc();
    }
    size_t cb = cfgs.size() * sizeof(gf_lxc_dev);
    bool changed = a->dirty || a->h_cfgs.size() != cb || a->h_slot_of.size() != slot_of.size() ||
                   (cb && memcmp(a->h_cfgs.data(), cfgs.data(), cb)) ||
                   memcmp(a->h_slot_of.data(), slot_of.data(), slot_of.size() * 2);
    if (changed) {
        if (getenv("GF_SYNC_DEBUG")) fprintf(stderr, "[gf] program table upload (dirty %d)\n", (int)a->dirty);
        if ((r = a->d_slot_of_lxc.ensure(65536 * 2))) return r;
        if ((r = a->d_cfgs.ensure(std::max<size_t>(1, cb)))) return r;
        a->h_cfgs.assign((const uint8_t *)cfgs.data(), (const uint8_t *)cfgs.data() + cb);
        a->h_slot_of = slot_of;
        if (hip_ok(hipMemcpyAsync(a->d_slot_of_lxc.p, a->h_slot_of.data(), 65536 * 2, hipMemcpyHostToDevice, s), "slots"))
            return -EIO;
        if (cb && hip_ok(hipMemcpyAsync(a->d_cfgs.p, a->h_cfgs.data(), cb, hipMemcpyHostToDevice, s), "cfgs"))
            return -EIO;
        if (hip_ok(hipStreamSynchronize(s), "cfg sync")) return -EIO;
        a->dirty = false;
    }
    return 0;
}

// The host's bound of a CT map's device count (ct_limits, lru_evict) tightened
// from the counts the recent eviction chains wrote to pinned host memory: the
// newest one whose event has fired (a query, never a wait), plus what the calls
// enqueued since may have added.  A ring of events, so a host that runs several
// calls ahead of the device still finds a fired one.
// wait: block on the oldest pending event instead (the device only has to reach
// that earlier call, not drain the queue) — ct_limits' alternative to a readback.
static void ct_count_refresh(Map &m, bool wait = false) {
    if (m.h_stamp) {                                    // the multi-map pass's stamp (no wait: read as it is)
        const unsigned long long v = *reinterpret_cast<volatile unsigned long long *>(m.h_stamp);
        const uint32_t seq = (uint32_t)(v >> 32), j = seq % Map::GF_STRING;
        if (seq > m.st_floor && m.st_seq[j] == seq)
            m.dev_count_hi = std::min<uint64_t>(m.dev_count_hi, (uint64_t)(uint32_t)v + (m.cnt_add - m.st_add[j]));
    }
    if (!m.ev_pending || !m.h_evcount) return;
    if (wait)
        for (uint32_t k = Map::GF_EVRING; k >= 1; k--) {
            const uint32_t j = (m.ev_head + Map::GF_EVRING - k) % Map::GF_EVRING;
            if (m.ev_pending & (1u << j)) { (void)hipEventSynchronize(m.ev_count[j]); break; }
        }
    for (uint32_t k = 1; k <= Map::GF_EVRING; k++) {
        const uint32_t j = (m.ev_head + Map::GF_EVRING - k) % Map::GF_EVRING;
        if (!(m.ev_pending & (1u << j))) continue;
        if (hipEventQuery(m.ev_count[j]) != hipSuccess) continue;
        m.dev_count_hi = std::min<uint64_t>(m.dev_count_hi, (uint64_t)m.h_evcount[j] + (m.cnt_add - m.ev_add[j]));
        // this slot and every older one are used up
        for (uint32_t q = k; q <= Map::GF_EVRING; q++) m.ev_pending &= ~(1u << ((m.ev_head + Map::GF_EVRING - q) % Map::GF_EVRING));
        return;
    }
}
// Element accounting mode of the CT maps for a batch of n packets inserting at
// most per_pkt entries each (see ingress_run); fills the launch descriptors.
static int ct_limits(const std::shared_ptr<Map> &ct4m, const std::shared_ptr<Map> &ct6m, uint32_t n, uint32_t per_pkt,
                     hipStream_t s, uint32_t &strict, gf_htab_desc &cfg_ct4, gf_htab_desc &cfg_ct6) {
    strict = 0;
    if (ct4m) cfg_ct4 = ct_dev_desc(*ct4m);
    if (ct6m) cfg_ct6 = ct_dev_desc(*ct6m);
    for (auto &m : {ct4m, ct6m}) {
        if (!m) continue;
        // LRU: never fails in the kernel (it evicts); here no eviction inside a classify
        // call, the entries stay until the eviction pass after it (lru_evict), bounded by
        // the slot array (7/8 load = 3.5 x max_entries)
        const uint64_t limit = dev_insert_limit(*m);
        if (m->host_valid) { m->dev_count_hi = m->ht.count; m->ev_pending = 0; m->st_floor = m->lru_seq; }
        ct_count_refresh(*m);
        // near the limit: the count of an eviction chain a few calls back first (no
        // queue drain), then, if that is not enough, a readback
        if (m->dev_count_hi + (uint64_t)per_pkt * n > limit && (uint64_t)per_pkt * n <= limit && !m->host_valid)
            ct_count_refresh(*m, true);
        // (no readback when the batch alone could exceed the limit: strict either way)
        if (m->dev_count_hi + (uint64_t)per_pkt * n > limit && (uint64_t)per_pkt * n <= limit && !m->host_valid) {
            if (getenv("GF_SYNC_DEBUG"))
                fprintf(stderr, "[gf] CT count readback (bound %llu + %u x %u > %llu)\n", (unsigned long long)m->dev_count_hi,
                        per_pkt, n, (unsigned long long)limit);
            uint32_t dc = 0;
            if (hip_ok(hipStreamSynchronize(s), "ct count sync") ||
                hip_ok(hipMemcpy(&dc, m->d_count.p, 4, hipMemcpyDeviceToHost), "read ct count"))
                return -EIO;
            m->dev_count_hi = dc;
            m->ev_pending = 0;
            m->st_floor = m->lru_seq;
        }
        if (m->dev_count_hi + (uint64_t)per_pkt * n > limit) strict |= m == ct4m ? 1u : 2u;
        m->dev_count_hi += (uint64_t)per_pkt * n;
        m->cnt_add += (uint64_t)per_pkt * n;
    }
    return 0;
}

// The CT maps the programs of a call bind, per family, each once.  pct: some family
// has more than one (endpoints with the ConntrackLocal option, cilium_ct4_<id>,
// pkg/endpoint/bpf.go:268-276) — the per-endpoint kernels (ing_ct<FAM, true>).
struct CtMaps {
    std::vector<std::shared_ptr<Map>> m4, m6;
    bool pct = false;
    std::shared_ptr<Map> one(int fam) const {
        const auto &v = fam == 6 ? m6 : m4;
        return v.empty() ? nullptr : v[0];
    }
};
static int ct_maps_of(const std::vector<std::shared_ptr<ProgLxc>> &progs, CtMaps &cm) {
    std::set<const Map *> s4, s6;
    for (auto &p : progs) {
        if (p->ct4 && s4.insert(p->ct4.get()).second) cm.m4.push_back(p->ct4);
        if (p->ct6 && s6.insert(p->ct6.get()).second) cm.m6.push_back(p->ct6);
    }
    for (auto *m : s4)
        if (s6.count(m)) return -EINVAL;                // one map bound as both families' CT map
    cm.pct = cm.m4.size() > 1 || cm.m6.size() > 1;
    return 0;
}
// Per-endpoint maps: each map's host bound moves as if the whole batch could insert
// into it; a family whose maps could any of them fill counts every insert exactly
// (strict: the count and insert limit the program table's descriptor carries,
// ct_dev_desc), else each lane adds its net inserts to its program's map
// (lane_flush_added).
static int ct_limits_pct(const CtMaps &cm, uint32_t n, uint32_t per_pkt, hipStream_t s, uint32_t &strict) {
    gf_htab_desc d4{}, d6{};
    int r;
    strict = 0;
    for (auto &m : cm.m4) {
        uint32_t st = 0;
        if ((r = ct_limits(m, nullptr, n, per_pkt, s, st, d4, d6))) return r;
        strict |= st;
    }
    for (auto &m : cm.m6) {
        uint32_t st = 0;
        if ((r = ct_limits(nullptr, m, n, per_pkt, s, st, d4, d6))) return r;
        strict |= st;
    }
    return 0;
}

// After ct_limits: the families (bit 0: IPv4, bit 1: IPv6) with a HASH map the batch could
// fill.  Such a map fails an insert at exactly max_entries, so which packet fails depends on
// the order of the inserts: the family runs in batch order (k_ing_serial_keys).  An LRU CT
// map never fails an insert (its strict mode only keeps the count exact).
static uint32_t ct_serial_fams(const CtMaps &cm) {
    uint32_t f = 0;
    for (auto &m : cm.m4)
        if (m->type != GF_MAP_TYPE_LRU_HASH && m->dev_count_hi > dev_insert_limit(*m)) f |= 1u;
    for (auto &m : cm.m6)
        if (m->type != GF_MAP_TYPE_LRU_HASH && m->dev_count_hi > dev_insert_limit(*m)) f |= 2u;
    return f;
}

// ---- CT sweeps on the device: per-map LRU state (histogram, cutoffs, log) and
// the cluster-start bits of the GC sweep.
static int ct_sweep_bufs(Map &m, LruDev *&L, uint32_t *&bits) {
    if (!m.d_lru.p) {
        if (m.d_lru.ensure(sizeof(LruDev))) return -ENOMEM;
        if (hip_ok(hipMemset(m.d_lru.p, 0, sizeof(LruDev)), "lru init")) return -EIO;
    }
    const size_t nw = (m.ht.nslots + 31) / 32;
    if (m.d_gcbits.bytes < nw * 4 && m.d_gcbits.ensure(nw * 4)) return -ENOMEM;
    L = (LruDev *)m.d_lru.p;
    bits = (uint32_t *)m.d_gcbits.p;
    return 0;
}
static void ct_sweep_launch(Map &m, LruDev *L, uint32_t *bits, hipStream_t s) {
    const gf_htab_desc d = m.hdesc();
    const uint32_t lt_off = m.ht.codec == GF_VCODEC_CT ? 0u : 32u;
    const uint64_t nw = (d.mask + 1 + 31) / 32;
    const uint32_t grid = (uint32_t)std::min<uint64_t>((nw + BLOCK - 1) / BLOCK, 65535u * 8);
    hipLaunchKernelGGL(k_gc_starts, dim3(grid), dim3(BLOCK), 0, s, d, bits, (const GcCut *)&L->cut);
    hipLaunchKernelGGL(k_gc_clusters, dim3(grid), dim3(BLOCK), 0, s, d, m.ht.mode, lt_off, (const GcCut *)&L->cut,
                       (const uint32_t *)bits, L->res);
}
// The LRU stand-in after a classify call (k_lru_*: see the kernels): fully on the
// device, a chain of launches that exit at once unless the map's count exceeds its
// high-water mark; not launched at all while the host's bound of the count is at or
// below it.
// One map's part of an eviction pass: its state, this call's count word, and the
// descriptor the kernels read (kind 0: nothing to launch for it).
struct LruPrep { Map *m = nullptr; int kind = 0; uint32_t slot = 0; LruMap lm{}; };
// track: the chain writes the count to the map's pinned ring behind an event, for the
// host's bound (the multi-map pass does not: one event record per map per call costs
// more host time than the bound saves there).
static int lru_prepare(const std::shared_ptr<Map> &m, LruPrep &P, bool track = true) {
    P = LruPrep{};
    if (!m || m->type != GF_MAP_TYPE_LRU_HASH || !m->d_slots.p) return 0;
    m->lru_seq++;
    ct_count_refresh(*m);
    if (m->dev_count_hi <= lru_high_water(m->max_entries)) return 0;   // cannot have crossed HW
    if (!m->d_lru.p) {
        if (m->d_lru.ensure(sizeof(LruDev))) return -ENOMEM;
        if (hip_ok(hipMemset(m->d_lru.p, 0, sizeof(LruDev)), "lru init")) return -EIO;
    }
    const gf_htab_desc d = m->hdesc();
    const int kind = d.slot_size == 32 && d.ksz == 14 && d.vin == 16 && d.voff == 16 ? 1
                   : d.slot_size == 64 && d.ksz == 40 && d.vin == 16 && d.voff == 48 ? 2 : 0;
    if (!kind) return -EIO;                              // the CT codec's layouts only
    if (!m->h_evcount) {
        // every event first, the count words last: a failure leaves nothing half made
        hipEvent_t ev[Map::GF_EVRING] = {};
        bool ok = true;
        for (auto &e : ev)
            if (ok && hip_ok(hipEventCreateWithFlags(&e, hipEventDisableTiming), "lru count event")) ok = false;
        void *p = nullptr;
        if (ok && hip_ok(hipHostMalloc(&p, 4 * Map::GF_EVRING, hipHostMallocMapped | hipHostMallocCoherent),
                         "lru count words"))
            ok = false;
        if (!ok) {
            for (auto &e : ev)
                if (e) (void)hipEventDestroy(e);
            return -ENOMEM;
        }
        uint32_t *dp = nullptr;
        if (hip_ok(hipHostGetDevicePointer((void **)&dp, p, 0), "lru count words")) {
            for (auto &e : ev) (void)hipEventDestroy(e);
            (void)hipHostFree(p);
            return -EIO;
        }
        for (uint32_t k = 0; k < Map::GF_EVRING; k++) m->ev_count[k] = ev[k];
        m->h_evcount = (uint32_t *)p;
        m->d_evcount = dp;
    }
    if (!track && !m->h_stamp) {
        void *p = nullptr;
        unsigned long long *dp = nullptr;
        if (hip_ok(hipHostMalloc(&p, 8, hipHostMallocMapped | hipHostMallocCoherent), "lru stamp")) return -ENOMEM;
        *(unsigned long long *)p = 0ull;
        if (hip_ok(hipHostGetDevicePointer((void **)&dp, p, 0), "lru stamp")) { (void)hipHostFree(p); return -EIO; }
        m->h_stamp = (unsigned long long *)p;
        m->d_stamp = dp;
    }
    P.m = m.get(); P.kind = kind; P.slot = m->ev_head;
    LruMap &M = P.lm;
    M.hcount = track ? m->d_evcount + P.slot : nullptr;
    M.stamp = track ? nullptr : m->d_stamp;
    if (!track) {                                       // the stamp's reference point: cnt_add at this call
        const uint32_t j = m->lru_seq % Map::GF_STRING;
        m->st_seq[j] = m->lru_seq;
        m->st_add[j] = m->cnt_add;
    }
    const uint64_t ns = d.mask + 1, spl = 128 / d.slot_size;
    M.d = d; M.L = (LruDev *)m->d_lru.p; M.nl = ns / spl; M.sl = lru_sample_lines(M.nl);
    M.mode = m->ht.mode; M.max_entries = m->max_entries; M.seq = m->lru_seq;
    return 0;
}
// After the chain: the count word's event, for the host's bound (ct_count_refresh).
static int lru_post(const LruPrep &P, uint32_t now, hipStream_t s) {
    Map *m = P.m;
    if (hip_ok(hipEventRecord(m->ev_count[P.slot], s), "lru count event")) return -EIO;
    m->ev_pending |= 1u << P.slot;
    m->ev_add[P.slot] = m->cnt_add;
    m->ev_head = (P.slot + 1) % Map::GF_EVRING;
    static const bool stats = getenv("GF_LRU_STATS") != nullptr;   // diagnostics: syncs the stream
    if (stats) {
        LruDev h;
        LruDev *L = P.lm.L;
        if (!hip_ok(hipMemcpyAsync(&h, L, offsetof(LruDev, log), hipMemcpyDeviceToHost, s), "lru stats") &&
            !hip_ok(hipStreamSynchronize(s), "lru stats") && h.nlog) {
            uint32_t n = h.nlog;
            LruLog g{};
            if (!hip_ok(hipMemcpy(&g, &L->log[std::min(n, GF_LRU_LOGCAP) - 1], sizeof g, hipMemcpyDeviceToHost),
                        "lru stats log") && g.seq == m->lru_seq)
                fprintf(stderr, "[lru] seq %u now %u: K %u es %llu lines %llu of %llu (hand %llu) evicted %llu "
                        "(rounds %llu / %llu / %llu), cleared %llu\n", g.seq, now, g.age_cut, h.es, g.lines,
                        (unsigned long long)P.lm.nl, g.hand, g.evicted, h.kills[0], h.kills[1], h.kills[2], h.cleared);
        }
    }
    return 0;
}
// The LRU stand-in after a classify call (k_lru_*: see the kernels): fully on the
// device, a chain of launches that exit at once unless the map's count exceeds its
// high-water mark; not launched at all while the host's bound of the count is at or
// below it.
static int lru_evict(const std::shared_ptr<Map> &m, uint32_t now, hipStream_t s) {
    LruPrep P;
    int r;
    if ((r = lru_prepare(m, P)) || !P.kind) return r;
    const LruMap &M = P.lm;
    const gf_htab_desc &d = M.d;
    LruDev *L = M.L;
    const int kind = P.kind;
    const uint64_t spl = 128 / d.slot_size, nl = M.nl, sl = M.sl;
    const uint32_t gs = (uint32_t)std::min<uint64_t>((sl * spl + GF_LRU_HB - 1) / GF_LRU_HB, resident_blocks(2));
    const uint32_t gh = resident_blocks(8);
    const uint32_t *cnt = (const uint32_t *)d.count;
    const uint32_t mx = M.max_entries, mode = M.mode;
    {
        ProfScope ps("k_lru_evict", s);
        // the window's sample and plan, then (large tables only) the whole-table
        // pair, which runs only when the window held no entry
        for (uint32_t wide = 0; wide < (sl < nl ? 2u : 1u); wide++) {
            const dim3 g(wide ? gh : gs);
            if (kind == 1)
                hipLaunchKernelGGL(k_lru_sample<1>, g, dim3(GF_LRU_HB), 0, s, d, mode, now, L, sl, mx, wide);
            else
                hipLaunchKernelGGL(k_lru_sample<2>, g, dim3(GF_LRU_HB), 0, s, d, mode, now, L, sl, mx, wide);
            hipLaunchKernelGGL(k_lru_plan, dim3(1), dim3(1024), 0, s, cnt, mx, L, sl, nl, wide);
        }
        for (uint32_t round = 0; round < GF_LRU_ROUNDS; round++) {
            // round 1 is rare and short (what round 0's estimate left): a smaller grid, the same chunks
            const dim3 g(round == 1 ? gh / 8 : gh);
            if (kind == 1) {
                hipLaunchKernelGGL((k_lru_hand<1, 0>), g, dim3(GF_LRU_HT), 0, s, d, mode, now, L, nl, sl, mx, round);
                hipLaunchKernelGGL((k_lru_hand<1, 1>), g, dim3(GF_LRU_HT), 0, s, d, mode, now, L, nl, sl, mx, round);
            } else {
                hipLaunchKernelGGL((k_lru_hand<2, 0>), g, dim3(GF_LRU_HT), 0, s, d, mode, now, L, nl, sl, mx, round);
                hipLaunchKernelGGL((k_lru_hand<2, 1>), g, dim3(GF_LRU_HT), 0, s, d, mode, now, L, nl, sl, mx, round);
            }
        }
        hipLaunchKernelGGL(k_lru_end, dim3(1), dim3(1), 0, s, d.count, M.seq, now, L, mx, nl, M.hcount);
    }
    if ((r = lru_post(P, now, s))) return r;
    return hip_ok(hipGetLastError(), "k_lru_evict");
}
// The pass over several maps (per-endpoint CT maps): the maps that may be above their
// high-water marks, GF_LRU_MULTI of one slot kind per chain of launches (a single one
// takes the one-map chain).  Each map's rounds, cutoffs and log are its own, exactly
// as with its own chain.
static int lru_evict_maps(const std::vector<std::shared_ptr<Map>> &ms, uint32_t now, hipStream_t s) {
    if (ms.empty()) return 0;
    if (ms.size() == 1) return lru_evict(ms[0], now, s);
    std::vector<LruPrep> ps;
    int r;
    for (auto &m : ms) {
        LruPrep P;
        if ((r = lru_prepare(m, P, false))) return r;
        if (P.kind) ps.push_back(P);
    }
    if (ps.empty()) return 0;
    const uint32_t gh = resident_blocks(8);
    ProfScope prof("k_lru_evict", s);
    for (int kind = 1; kind <= 2; kind++) {
        std::vector<const LruPrep *> ks;
        for (auto &P : ps)
            if (P.kind == kind) ks.push_back(&P);
        for (size_t b = 0; b < ks.size(); b += GF_LRU_MULTI) {
            LruBatch B{};
            B.n = (uint32_t)std::min<size_t>(GF_LRU_MULTI, ks.size() - b);
            uint64_t gs = 1;
            bool big = false;
            for (uint32_t k = 0; k < B.n; k++) {
                B.m[k] = ks[b + k]->lm;
                const uint64_t spl = 128 / B.m[k].d.slot_size;
                gs = std::max<uint64_t>(gs, (B.m[k].sl * spl + GF_LRU_HB - 1) / GF_LRU_HB);
                big |= B.m[k].sl < B.m[k].nl;
            }
            const dim3 g1((uint32_t)std::min<uint64_t>(gs, resident_blocks(2)));
            for (uint32_t wide = 0; wide < (big ? 2u : 1u); wide++) {
                // (the whole-table pass runs only for a map whose window held no entry: a
                // smaller grid, which costs little on the many calls where it has no work)
                const dim3 g(wide ? std::max<uint32_t>(gh / 8, 1) : g1.x);
                if (kind == 1) hipLaunchKernelGGL(k_lru_sample_multi<1>, g, dim3(GF_LRU_HB), 0, s, B, now, wide);
                else hipLaunchKernelGGL(k_lru_sample_multi<2>, g, dim3(GF_LRU_HB), 0, s, B, now, wide);
                hipLaunchKernelGGL(k_lru_plan_multi, dim3(B.n), dim3(1024), 0, s, B, wide);
            }
            for (uint32_t round = 0; round < GF_LRU_ROUNDS; round++) {
                // rounds 1 and 2 run only for what round 0's estimate left: smaller grids
                const dim3 g(round ? std::max<uint32_t>(gh / 8, 1) : gh);
                if (kind == 1) {
                    hipLaunchKernelGGL((k_lru_hand_multi<1, 0>), g, dim3(GF_LRU_HT), 0, s, B, now, round);
                    hipLaunchKernelGGL((k_lru_hand_multi<1, 1>), g, dim3(GF_LRU_HT), 0, s, B, now, round);
                } else {
                    hipLaunchKernelGGL((k_lru_hand_multi<2, 0>), g, dim3(GF_LRU_HT), 0, s, B, now, round);
                    hipLaunchKernelGGL((k_lru_hand_multi<2, 1>), g, dim3(GF_LRU_HT), 0, s, B, now, round);
                }
            }
            hipLaunchKernelGGL(k_lru_end_multi, dim3(1), dim3(64), 0, s, B, now);
            if ((r = hip_ok(hipGetLastError(), "k_lru_*_multi"))) return r;
        }
    }
    return 0;
}

// A mixed array's packets of programs without conntrack out of the schedule (ws().keys).
static int noct_mark(const std::shared_ptr<PolicyArray> &a, uint32_t n, hipStream_t s, bool wide = false) {
    Workspace &w = ws();
    ProfScope ps("k_ing_noct_mark", s);
    hipLaunchKernelGGL(k_ing_noct_mark, dim3((n + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, s, n, (const gf_rec *)w.rec.p,
                       (const gf_lxc_dev *)a->d_cfgs.p, (uint32_t *)w.keys.p, gf_key_for(n, wide));
    return hip_ok(hipGetLastError(), "k_ing_noct_mark");
}

// k_ing_pack over the columns: the records and bucket keys of ws() (ingress_run without a front,
// ingress_prepare).
static int pack_cols(const std::shared_ptr<PolicyArray> &a, const gf_pkt_cols *pkts, hipStream_t s) {
    Workspace &w = ws();
    const uint32_t n = pkts->n;
    ProfScope ps("k_ing_pack", s);
    hipLaunchKernelGGL(k_ing_pack, dim3((n + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, s, *pkts,
                       (const uint16_t *)a->d_slot_of_lxc.p, (gf_rec *)w.rec.p, (uint32_t *)w.keys.p, gf_key_for(n));
    return hip_ok(hipGetLastError(), "k_ing_pack");
}

// What the launches of k_ing_groups / k_ing_groups_dbg over the two families share.
struct IngLaunch {
    uint32_t grid;
    hipStream_t s;
    const Workspace &w;
    const IngCtx &X;
    gf_ingress_out *out;
    unsigned long long *sink;
    uint4 *dlog;                   // a program with DEBUG: the instantiations that log (else null)
    bool pct;                      // per-endpoint CT maps (ConntrackLocal)
    bool pol_wave;                 // the egress deliveries' pass (single-packet buckets): IPv4 only, IPv6 has
                                   // no such instantiation and runs the plain kernel
};
// One family's launch; cnt: the family's CT map's count word (non-strict mode accounts the kernel's
// net element change there), null with per-endpoint maps.
template <int FAM>
static void launch_ing_groups(const IngLaunch &g, uint32_t *cnt) {
    const Workspace &w = g.w;
    auto go = [&](auto kern, auto... dlog) {
        hipLaunchKernelGGL(kern, dim3(g.grid), dim3(BLOCK), 0, g.s, g.X, (uint32_t *)w.sched.p, (const uint2 *)w.order.p,
                           (const uint32_t *)w.perm.p, (const gf_rec *)w.rec.p, g.out, cnt, g.sink,
                           dlog...);
    };
    ProfScope ps(FAM == 6 ? "k_ing_groups6" : "k_ing_groups", g.s);
    if (g.dlog && g.pct) go(k_ing_groups_dbg<FAM, true>, g.dlog);
    else if (g.dlog) go(k_ing_groups_dbg<FAM, false>, g.dlog);
    else if (g.pct) go(k_ing_groups<FAM, 1, true>);
    else if (FAM == 4 && g.pol_wave) go(k_ing_groups<4, GF_GRAB_ING, false, true>);
    else go(k_ing_groups<FAM>);
}

// handle_policy over a batch: the program table, the CT maps' accounting, the flow-group schedule,
// the group kernels, then the proxy log, the notifications and the LRU stand-in.
static int ingress_run(const std::shared_ptr<PolicyArray> &a, const gf_pkt_cols *pkts, uint32_t now_sec, hipStream_t s,
                       const PolicyPass &P) {
    int r;
    const bool plain = P.kind == PassKind::Plain, egress = P.kind == PassKind::Egress;
    // the frame fronts and the egress front write saddr6 | daddr6 of a packet as one 32-B piece;
    // the plain call reads two columns
    const uint32_t a6_stride = plain ? 16u : 32u;
    // the frame fronts' keys (gf_key_for(n, true))
    const bool wide = P.kind == PassKind::Frames;
    // the egress deliveries' pass: single-packet buckets in packet-index order, the IPv4 kernel that
    // takes them a wave at a time
    const bool pol_wave = egress;
    // a frame entry's records are written whole (no read-modify-write) unless its front left a flag
    // in them (keep_flags)
    const bool pout_wo = P.pout && P.kind == PassKind::Frames && !P.keep_flags;
    const int noct = array_noct(a);                     // programs without conntrack: 0 none, 1 some, 2 all
    if (noct && egress) return -EOPNOTSUPP;             // (the egress entry point refuses such arrays)
    // trace notifications: the plain call decides and prepares here, the frame and egress
    // callers (whose earlier kernels mark packets) pass their decision
    const bool tracing = plain ? event_ring().records && array_traces(a) : P.on;
    if (tracing && plain && (r = trace_prepare(pkts->n, false, s))) return r;
    // debug notifications (GF_LXC_F_DEBUG): the plain call only; every other entry point runs
    // such programs as if the flag were clear
    const bool debugging = plain && event_ring().records && a->dbg && noct != 2;
    if (debugging && (r = dbg_prepare(pkts->n, s))) return r;
    gf_ingress_out *const out = P.out;
    uint8_t *const pout = P.pout;
    // 1. sync tables, build the device program table
    std::vector<std::shared_ptr<ProgLxc>> progs;
    host_mark("ing");
    if ((r = prog_table(a, s, progs))) return r;
    host_mark("prog");
    // CT maps: the global layout (every program binds cilium_ct4_global / ct6_global)
    // or per-endpoint maps (ConntrackLocal, ct_maps_of: the PCT kernels)
    CtMaps cm;
    if ((r = ct_maps_of(progs, cm))) return r;
    std::shared_ptr<Map> ct4m = cm.pct ? nullptr : cm.one(4), ct6m = cm.pct ? nullptr : cm.one(6);
    // Strict (exact, atomic per insert) element accounting only when this batch could
    // reach the limit.  HASH maps are limited by max_entries (E2BIG).  LRU maps never
    // fail in the kernel (they evict); here they keep entries past max_entries until
    // GC and are bounded only by the slot array (7/8 load), see DESIGN.md.
    // The decision uses a host-side upper bound of the device element count (each
    // packet inserts at most 2 entries), read back from the device only when the
    // bound gets near the limit — steady-state batches never wait on the GPU here.
    // Per-endpoint maps: the same per family, over every map of it (ct_limits_pct).
    uint32_t strict = 0;
    gf_htab_desc cfg_ct4{}, cfg_ct6{};
    if ((r = ct_limits(ct4m, ct6m, pkts->n, 2, s, strict, cfg_ct4, cfg_ct6))) return r;
    if (cm.pct && (r = ct_limits_pct(cm, pkts->n, 2, s, strict))) return r;
    host_mark("ctlim");
    // 2. group by flow group (records and keys first), 3. longest-first bucket order
    uint32_t n = pkts->n;
    // A family with a HASH map that could fill: one bucket, in batch order (a schedule
    // built ahead of the call is rebuilt here)
    const uint32_t serial = n > 1 && noct != 2 ? ct_serial_fams(cm) : 0u;
    const bool prepared = P.prepared && !serial;
    Workspace &w = ws();
    if (prepared) {
        // pack + schedule already built in ws() (ingress_prepare)
    } else if ((r = ws_grow(n))) {
        return r;
    } else if (P.pack) {
        if ((r = P.pack((const uint16_t *)a->d_slot_of_lxc.p, (gf_rec *)w.rec.p, (uint32_t *)w.keys.p))) return r;
    } else if ((r = pack_cols(a, pkts, s))) {
        return r;
    }
    host_mark("pack");
    // Programs without conntrack: their packets leave the schedule (mixed array), or
    // there is no schedule at all (every program; k_ing_noct alone, below)
    if (noct == 1 && !prepared && (r = noct_mark(a, n, s, wide))) return r;
    if (serial) {
        ProfScope ps("k_ing_serial_keys", s);
        hipLaunchKernelGGL(k_ing_serial_keys, dim3(grid_for(n)), dim3(BLOCK), 0, s, n, (uint32_t *)w.keys.p,
                           gf_key_for(n, wide), serial);
        if ((r = hip_ok(hipGetLastError(), "k_ing_serial_keys"))) return r;
    }
    if (!prepared && noct != 2 && (r = schedule_groups(n, s, egress, wide))) return r;
    host_mark("sched");
    // 4. handle_policy: one bucket per lane, buckets from the longest-first queue
    IngCtx X{};
    X.cfgs = (const gf_lxc_dev *)a->d_cfgs.p;
    X.saddr6 = pkts->saddr6; X.daddr6 = pkts->daddr6;
    X.a6_stride = a6_stride;
    if (ct4m) X.ct4 = cfg_ct4;
    if (ct6m) X.ct6 = cfg_ct6;
    X.now = now_sec; X.host_ifindex = host_ifindex();
    X.strict = strict;
    X.pout = pout;
    X.pout_wo = pout_wo ? 1u : 0u;
    X.pol_wave = pol_wave ? 1u : 0u;
    X.snap = P.wsnap; X.snap_stride = P.ev_stride;
    const gf_node_cfg &node = node_cfg();
    X.gw = node.ipv4_gateway;
    memcpy(X.host6, node.host_ip6, 16);
    if (tracing) { X.tmark = (uint8_t *)trace_ws().mark.p; X.tcap = (uint8_t *)trace_ws().px.p; }
    X.rlog = P.rlog; X.rlog_n = P.rlog_n; X.rlog_off = P.rlog_off; X.rs = P.rs;
    if ((r = px_log_begin(n, s, X, P.px_keep))) return r;
    unsigned long long *sink = (unsigned long long *)stats_sink();
    if (noct != 2) {
        // resident-grid launches: every wave loops on its family's queue until it is drained
        const uint32_t grid = std::min(resident_blocks(8), (n + BLOCK - 1) / BLOCK);
        const IngLaunch g{grid, s, w, X, out, sink, debugging ? (uint4 *)dbg_ws().log.p : nullptr, cm.pct, pol_wave};
        launch_ing_groups<4>(g, ct4m ? (uint32_t *)ct4m->d_count.p : nullptr);
        // IPv6 packets reach conntrack only with v6 columns
        if (pkts->saddr6) launch_ing_groups<6>(g, ct6m ? (uint32_t *)ct6m->d_count.p : nullptr);
    }
    if ((r = hip_ok(hipGetLastError(), "k_ing_groups"))) return r;
    if (noct) {
        ProfScope ps("k_ing_noct", s);
        hipLaunchKernelGGL(k_ing_noct, dim3((n + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, s, X, n, noct == 2 ? 1u : 0u,
                           (const gf_rec *)w.rec.p, out, sink);
        if ((r = hip_ok(hipGetLastError(), "k_ing_noct"))) return r;
    }
    host_mark("groups");
    const uint32_t *ev_len = P.ev_len ? P.ev_len : pkts->len;
    if ((r = px_log_apply(X, s, P.wsnap, ev_len, P.ev_stride, pout ? pout : (uint8_t *)out, pout != nullptr, n))) return r;
    {
        EvSrc E{};
        E.recs = pout ? pout : (const uint8_t *)out;
        E.stride = pout ? 24u : 8u; E.act_off = pout ? 1u : 0u; E.stage_off = pout ? 0 : -1;
        E.prec = (const gf_rec *)w.rec.p; E.cfgs = (const gf_lxc_dev *)a->d_cfgs.p;
        E.len = ev_len; E.flow_hash = pkts->flow_hash; E.n = n;
        E.snap = P.ev_snap; E.snap_stride = P.ev_stride;
        if (tracing) {
            const TraceWs &t = trace_ws();
            E.trace = 1; E.kind = (uint32_t)P.kind;
            E.tmark = (const uint8_t *)t.mark.p; E.tcap_px = (const uint8_t *)t.px.p;
            E.tcap_in = (const uint8_t *)t.in.p;
            E.host_ifindex = host_ifindex(); E.encap_ifindex = node.encap_ifindex;
            E.nd_trace = P.nd_trace; E.nd_ifindex = P.nd_ifindex;
            E.orig = P.orig; E.lxc_id = P.lxc_id;
            E.hmark = P.hmark;
            if (!plain) E.slot_of = (const uint16_t *)a->d_slot_of_lxc.p;
        }
        if (debugging) { E.dlog = (const uint4 *)dbg_ws().log.p; E.tc_index = pkts->tc_index; E.host_ifindex = host_ifindex(); }
        if ((r = emit_drop_events(E, s, debugging))) return r;
    }
    host_mark("px+ev");
    for (auto &p : progs) {
        if (p->policy) p->policy->device_modified();
    }
    if (P.lru && ((r = lru_evict_maps(cm.m4, now_sec, s)) || (r = lru_evict_maps(cm.m6, now_sec, s)))) return r;
    host_mark("lru");
    for (auto *v : {&cm.m4, &cm.m6})
        for (auto &m : *v) m->device_modified();
    return 0;
}

// The stateless half of ingress_run (k_ing_pack + the flow-group schedule) into ws().
static int ingress_prepare(const std::shared_ptr<PolicyArray> &a, const gf_pkt_cols *pkts, hipStream_t s) {
    const uint32_t n = pkts->n;
    int r;
    if ((r = ws_grow(n)) || (r = pack_cols(a, pkts, s))) return r;
    const int noct = array_noct(a);
    if (noct == 2) return 0;                            // no program with conntrack: no schedule
    if (noct == 1 && (r = noct_mark(a, n, s))) return r;
    return schedule_groups(n, s);
}

// The stream that builds the next batch's schedule, and the events between the two.
struct PipeSync {
    hipStream_t aux = nullptr;
    hipEvent_t ready = nullptr, built[2] = {nullptr, nullptr}, done[2] = {nullptr, nullptr};
    int init() {
        if (aux) return 0;
        if (hip_ok(hipStreamCreateWithFlags(&aux, hipStreamNonBlocking), "aux stream")) return -EIO;
        for (hipEvent_t *e : {&ready, &built[0], &built[1], &done[0], &done[1]})
            if (hip_ok(hipEventCreateWithFlags(e, hipEventDisableTiming), "pipe event")) return -EIO;
        return 0;
    }
};
static PipeSync &pipe_sync() { static const char tag = 0; return cur_ctx().get<PipeSync>(&tag); }

// ---- what the frame entry points (pipeline, from-overlay, from-host) share on the host
// The frames and outputs of a classify call: 1 to go on, 0 for an empty batch, or -errno.
// cols_ok: the output and the entry's own required columns are there.
static int frames_check(const gf_frames &fr, bool cols_ok) {
    if (fr.n == 0) return 0;
    if (!fr.snap || !fr.len || !cols_ok) return -EFAULT;
    if (fr.snap_stride < 14 || fr.snap_stride > 256) return -EINVAL;   // a header snap, staged in LDS
    if (fr.n > (1u << 30)) return -E2BIG;
    return 1;
}

// A 20-byte-key table's IPv4 keys as an address set, or null (GF_XDP_NOSETS: diagnosis, the hash table)
static void front_addr_set(const std::shared_ptr<Map> &m, hipStream_t s, const uint32_t *&set, uint32_t &bits,
                           uint32_t &zero) {
    if (getenv("GF_XDP_NOSETS") || m->addr_set(20, 8192, s, &set, &bits, &zero)) set = nullptr;
}
static LxcDev lxc_dev(const std::shared_ptr<Map> &m, hipStream_t s) {
    LxcDev d{};
    d.lxc = m->hdesc();
    front_addr_set(m, s, d.lxset, d.lxbits, d.lxzero);
    return d;
}
// tun: the node's tunnel map, pushed; without it, or without ENCAP_IFINDEX, nothing is looked up
static EncapDev encap_dev(const gf_node_cfg &node, const std::shared_ptr<Map> &tun, hipStream_t s) {
    EncapDev d{};
    d.encap_ifindex = node.encap_ifindex;
    if (tun && node.encap_ifindex) {
        d.tunnel = tun->hdesc();
        front_addr_set(tun, s, d.tnset, d.tnbits, d.tnzero);
    }
    d.cluster_range = node.ipv4_cluster_range; d.cluster_mask = node.ipv4_cluster_mask; d.ipv4_mask = node.ipv4_mask;
    memcpy(d.node6, node.router_ip6, 12);
    return d;
}

// A frame kernel's launch: 256 lanes per block up to 128-B snaps, 128 lanes up to 256 B
// (<= 32 KiB of LDS rows), one tile per block
struct FrontLaunch {
    uint32_t nt, grid;
    size_t lds;
    hipStream_t s;
    unsigned long long *sink;
    uint8_t *s6, *d6;              // the fronts: saddr6 | daddr6 per packet in one 32-B piece (IngCtx::a6_stride 32)
    gf_key_cfg K;                  // the fronts: the bucket keys' width
};
// The geometry over fr.  vec_copy: the kernel's snap copy in 16-B pieces (the stride and both
// buffers allow it).
static FrontLaunch front_geometry(const gf_frames &fr, const uint8_t *snap_out, hipStream_t s, uint32_t &vec_copy) {
    FrontLaunch f{};
    f.nt = fr.snap_stride <= 128 ? 256u : 128u;
    f.grid = (fr.n + f.nt - 1) / f.nt;
    f.lds = (size_t)f.nt * fr.snap_stride;
    f.s = s;
    f.sink = (unsigned long long *)stats_sink();
    vec_copy = (fr.snap_stride % 16 == 0) && (((uintptr_t)fr.snap | (uintptr_t)snap_out) & 15u) == 0;
    return f;
}
template <class Kern, class... A>
static void launch_nt(Kern k256, Kern k128, const FrontLaunch &f, A... args) {
    if (f.nt == 256) hipLaunchKernelGGL(k256, dim3(f.grid), dim3(256), f.lds, f.s, args...);
    else hipLaunchKernelGGL(k128, dim3(f.grid), dim3(128), f.lds, f.s, args...);
}

// A frame entry point's run, under the caller's locks and after frames_check: the launch
// geometry, the IPv6 address buffer, the trace set-up, then ingress_run with launch(f, slot_of,
// rec, keys) as its front.  pass: the entry's own fields set (keep_flags, hmark), the rest filled
// here.  trace: the program's TR_FROM_* | its stage << 8 when it traces, else 0.  vec_copy /
// tcap_in: the entry descriptor's fields, set here before the launch.
template <class Launch>
static int front_call(const std::shared_ptr<PolicyArray> &policy, const gf_frames &fr, const uint32_t *flow_hash,
                      uint32_t now_sec, gf_pipeline_out *out, uint8_t *snap_out, hipStream_t s, PolicyPass &pass,
                      uint32_t trace, uint32_t ifindex, uint32_t &vec_copy, uint8_t *&tcap_in, const char *kernel,
                      Launch launch) {
    int r;
    const uint32_t n = fr.n;
    FrontLaunch f = front_geometry(fr, snap_out, s, vec_copy);
    PipeWs &w = pipe_ws();
    if (w.s6.bytes < (size_t)n * 32 && (r = w.s6.ensure((size_t)n * 32))) return r;
    f.s6 = (uint8_t *)w.s6.p; f.d6 = f.s6 + 16;
    f.K = gf_key_for(n, true);
    pass.kind = PassKind::Frames;                      // records completed as the pipeline's
    pass.nd_trace = trace;
    pass.nd_ifindex = ifindex;
    pass.on = event_ring().records && (trace || array_traces(policy));
    if (pass.on && (r = trace_prepare(n, trace != 0, s))) return r;
    if (pass.on && trace) tcap_in = (uint8_t *)trace_ws().in.p;
    gf_pkt_cols c2{};
    c2.n = n;
    c2.saddr6 = f.s6; c2.daddr6 = f.d6;
    c2.flow_hash = flow_hash;
    pass.pack = [&](const uint16_t *slot_of, gf_rec *rec, uint32_t *keys) -> int {
        ProfScope ps(kernel, s);
        launch(f, slot_of, rec, keys);
        return hip_ok(hipGetLastError(), kernel);
    };
    pass.pout = (uint8_t *)out;
    pass.ev_len = fr.len;
    pass.ev_snap = snap_out ? snap_out : fr.snap;
    pass.ev_stride = fr.snap_stride;
    pass.wsnap = snap_out;
    return ingress_run(policy, &c2, now_sec, s, pass);
}

// ---- host: the entry points over ingress_run, and the CT / proxy GC calls ----
#include "gf_host_entry.h"


// ---- the maps' bulk paths: k_bulk_*, gf_map_update_batch; k_dump_gather, gf_map_lookup_batch ----
#include "gf_map_bulk.h"

// ---- host: from-container: EgWs, k_eg_init, egress_call, gf_lxc_egress_classify ----
#include "gf_host_egress.h"

// ---- the ARP / ICMPv6 responder tail calls: k_respond, gf_respond ----
#include "gf_respond.h"

// ---- VXLAN / Geneve on the wire: k_tun_encap, k_tun_decap, gf_tunnel_* ----
#include "gf_tunnel.h"

// ---- draining the event ring with cilium monitor's filters: k_evd_*, gf_event_drain ----
#include "gf_events.h"

// ---- the prefilter over raw frames: k_xdpf_*, gf_xdp_filter_frames ----
#include "gf_xdp_frames.h"

// ---- forwarding the verdicts: k_fwd_*, gf_forward_queues, gf_forward_frames ----
#include "gf_forward.h"
