// gf_tunnel.h — VXLAN / Geneve on the wire (included at the end of gf_kernels.hip:
// kernels and the host side of gf_tunnel_load / gf_tunnel_encap / gf_tunnel_select /
// gf_tunnel_decap).
//
// The reference has no encapsulation code: the kernel's cilium_vxlan / cilium_geneve
// device does it (bpf/init.sh:295-300).  The headers follow RFC 791, RFC 768, RFC 7348
// section 5 and RFC 8926 section 3.4; the rules are in include/gpuflow.h.
//
// Both kernels are row copies whose byte shift (50 + opt_len on transmit, the outer
// header length on receive) is 2 mod 4, never a multiple of 16.  The tile is
// k_lb_frames': a block's rows staged in LDS by coalesced 16-byte loads, the headers
// built or parsed there, the shifted rows written by coalesced 16-byte stores.  A store
// piece is put together from five LDS dwords (v_alignbit), so the output needs no LDS
// image of its own beyond the header pieces.  R rows per 256-lane block, by stride class.
// The one's-complement sum is taken by a group of 8 lanes per frame over consecutive
// dwords (conflict-free), reduced with three __shfl_xor (DESIGN.md has the reasoning
// against one lane per frame).
#pragma once

struct TunDev {
    uint32_t flags, local_ip, dst_port, sport_min, sport_span, ttl, tos;
    uint32_t smac[2], dmac[2];         // LE words: bytes 0-3, 4-5
    uint32_t vec_in, vec_out;          // 16-byte loads of the input rows / stores of the inner rows allowed
};
#define TUN_NT 256

__device__ __forceinline__ uint32_t tun_sw16(uint32_t x) { return ((x & 0xffu) << 8) | ((x >> 8) & 0xffu); }
// the 16-bit one's-complement fold of a sum of 16-bit words (not complemented, unlike ck_fold)
__device__ __forceinline__ uint32_t tun_fold(uint32_t x) {
    x = (x & 0xffffu) + (x >> 16);
    return (x & 0xffffu) + (x >> 16);
}
// four bytes at any byte offset of an LDS image, little-endian
__device__ __forceinline__ uint32_t tun_ld32(const uint32_t *lds, uint32_t off) {
    const uint32_t q = off >> 2;
    return __funnelshift_r(lds[q], lds[q + 1], (off & 3u) * 8u);
}
// sixteen bytes at a byte offset that is 2 mod 4
__device__ __forceinline__ uint4 tun_ld128h(const uint32_t *lds, uint32_t off) {
    const uint32_t *p = lds + (off >> 2);
    const uint32_t d0 = p[0], d1 = p[1], d2 = p[2], d3 = p[3], d4 = p[4];
    return make_uint4(__funnelshift_r(d0, d1, 16), __funnelshift_r(d1, d2, 16), __funnelshift_r(d2, d3, 16),
                      __funnelshift_r(d3, d4, 16));
}
// 16-bit one's-complement partial sum (little-endian words) of bytes [off, end) of an LDS image,
// lane g of a group of 8 taking every 8th dword; off is even
__device__ __forceinline__ uint32_t tun_sum8(const uint32_t *lds, uint32_t off, uint32_t end, uint32_t g) {
    uint32_t s = 0;
    for (uint32_t a = off + 4u * g; a < end; a += 32u) {
        uint32_t w = tun_ld32(lds, a);
        const uint32_t rem = end - a;
        if (rem < 4u) w &= (1u << (8u * rem)) - 1u;
        s += (w & 0xffffu) + (w >> 16);
    }
    return s;
}
__device__ __forceinline__ uint32_t tun_group_sum(uint32_t s) {
    s += (uint32_t)__shfl_xor((int)s, 1);
    s += (uint32_t)__shfl_xor((int)s, 2);
    s += (uint32_t)__shfl_xor((int)s, 4);
    return s;
}
// up to 16 bytes of v to dst: one 16-byte store for a whole piece, bytes for a row's last one
__device__ __forceinline__ void tun_store_piece(uint8_t *dst, const uint4 &v, uint32_t nbytes, bool vec) {
    if (nbytes >= 16u && vec) { *reinterpret_cast<uint4 *>(dst) = v; return; }
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    for (uint32_t k = 0; k < 16u && k < nbytes; k++) dst[k] = (uint8_t)(w[k >> 2] >> (8u * (k & 3u)));
}
__host__ __device__ __forceinline__ uint32_t tun_in_pitch(uint32_t S) { return ((S + 3u) & ~3u) + 32u; }
__host__ __device__ __forceinline__ uint32_t tun_rx_pitch(uint32_t S) { return ((S + 15u) & ~15u) + 16u; }

// LDS of a block: the staged input rows (pitch tun_in_pitch: + 8 dwords, so the 8-lane groups of
// consecutive rows start on different banks), the header pieces of the output rows (pitch HP: + 16 B
// for the lane-per-frame header stores), and three words per row.
template <bool GENEVE, bool CSUM, int R>
__global__ __launch_bounds__(TUN_NT) void k_tun_encap(gf_tunnel_tx b, TunDev T, uint8_t *out, uint32_t out_stride,
                                                      uint32_t *out_len, uint8_t *status) {
    extern __shared__ __attribute__((aligned(16))) uint4 tun_lds[];
    constexpr uint32_t HP = GENEVE ? 144u : 80u;        // 50 + 64 B of headers end in piece 7; 50 B in piece 3
    const uint32_t S = b.frames.snap_stride, IP = tun_in_pitch(S);
    uint32_t *in32 = reinterpret_cast<uint32_t *>(tun_lds);
    uint8_t *in8 = reinterpret_cast<uint8_t *>(tun_lds);
    uint32_t *hd32 = in32 + (size_t)R * IP / 4;
    uint32_t *m_ovh = hd32 + (size_t)R * HP / 4, *m_len = m_ovh + R, *m_sum = m_len + R;
    const uint32_t tid = threadIdx.x;
    const uint32_t b0 = blockIdx.x * R;
    const uint32_t nb = b.frames.n - b0 < (uint32_t)R ? b.frames.n - b0 : (uint32_t)R;

    // ---- the status of each frame; only OK rows are staged, built and stored
    uint32_t ol = 0;
    if (tid < nb) {
        const uint32_t i = b0 + tid, len = b.frames.len[i];
        uint32_t st = GF_TUN_ST_OK;
        if (b.select && !b.select[i]) st = GF_TUN_ST_SKIPPED;
        else if (len < 14u) st = GF_TUN_ST_SHORT;
        else {
            if (GENEVE && b.opt) {
                ol = b.opt_len[i];
                if ((ol & 3u) || ol > b.opt_stride || ol > 64u) st = GF_TUN_ST_BAD_OPT;
            }
            if (CSUM && st == GF_TUN_ST_OK && len > S) st = GF_TUN_ST_TRUNCATED;
        }
        status[i] = (uint8_t)st;
        out_len[i] = st == GF_TUN_ST_OK ? len + 50u + ol : 0u;
        m_ovh[tid] = st == GF_TUN_ST_OK ? 50u + ol : 0u;
        m_len[tid] = len;
    }
    __syncthreads();
    // ---- stage the OK rows
    {
        const uint8_t *src = b.frames.snap + (size_t)b0 * S;
        if (T.vec_in) {
            const uint32_t per = S / 16u;
            for (uint32_t k = tid; k < nb * per; k += TUN_NT) {
                const uint32_t r = k / per, j = k - r * per;
                if (m_ovh[r]) tun_lds[(size_t)r * (IP / 16u) + j] = reinterpret_cast<const uint4 *>(src)[k];
            }
        } else {
            for (uint32_t k = tid; k < nb * S; k += TUN_NT) {
                const uint32_t r = k / S, j = k - r * S;
                if (m_ovh[r]) in8[(size_t)r * IP + j] = src[k];
            }
        }
    }
    __syncthreads();
    // ---- one lane per frame: the outer headers, as little-endian dwords of the row
    if (tid < nb && m_ovh[tid]) {
        const uint32_t i = b0 + tid, len = m_len[tid];
        uint32_t *h = hd32 + (size_t)tid * (HP / 4u);
        const uint32_t tot = (len + 36u + ol) & 0xffffu, ulen = (len + 16u + ol) & 0xffffu;
        const uint32_t ipid = b.ip_id ? b.ip_id[i] : 0u;
        const uint32_t frag = (T.flags & GF_TUN_F_DF) ? 0x4000u : 0u;
        const uint32_t src = T.local_ip, dst = b.remote_ip[i];
        const uint32_t fh = b.flow_hash ? b.flow_hash[i] : 0u;
        const uint32_t sport = T.sport_min + (uint32_t)(((uint64_t)fh * T.sport_span) >> 32);
        const uint32_t vni = b.tunnel_id[i] & 0xffffffu;
        uint32_t dm0 = T.dmac[0], dm1 = T.dmac[1];
        if (b.dst_mac) {
            const uint8_t *m = b.dst_mac + (size_t)i * 6;
            dm0 = (uint32_t)m[0] | ((uint32_t)m[1] << 8) | ((uint32_t)m[2] << 16) | ((uint32_t)m[3] << 24);
            dm1 = (uint32_t)m[4] | ((uint32_t)m[5] << 8);
        }
        // RFC 791 section 3.1: the header checksum over the ten 16-bit words, checksum field zero
        const uint32_t ipsum = ~tun_fold((0x4500u | T.tos) + tot + ipid + frag + ((T.ttl << 8) | 17u) + (src >> 16) +
                                        (src & 0xffffu) + (dst >> 16) + (dst & 0xffffu)) & 0xffffu;
        // the tunnel header as four big-endian words
        const uint32_t t0 = GENEVE ? ((ol >> 2) << 8) : 0x0800u, t1 = GENEVE ? 0x6558u : 0u;
        const uint32_t t2 = vni >> 8, t3 = (vni & 0xffu) << 8;
        h[0] = dm0;
        h[1] = (dm1 & 0xffffu) | (T.smac[0] << 16);
        h[2] = (T.smac[0] >> 16) | (T.smac[1] << 16);
        h[3] = 0x0008u | (0x45u << 16) | (T.tos << 24);
        h[4] = tun_sw16(tot) | (tun_sw16(ipid) << 16);
        h[5] = tun_sw16(frag) | (T.ttl << 16) | (17u << 24);
        h[6] = tun_sw16(ipsum) | (tun_sw16(src >> 16) << 16);
        h[7] = tun_sw16(src & 0xffffu) | (tun_sw16(dst >> 16) << 16);
        h[8] = tun_sw16(dst & 0xffffu) | (tun_sw16(sport) << 16);
        h[9] = tun_sw16(T.dst_port) | (tun_sw16(ulen) << 16);
        h[10] = tun_sw16(t0) << 16;                     // UDP checksum 0 for now
        h[11] = tun_sw16(t1) | (tun_sw16(t2) << 16);
        // RFC 768: pseudo-header (addresses, protocol, UDP length) and the UDP + tunnel headers
        uint32_t hs = (src >> 16) + (src & 0xffffu) + (dst >> 16) + (dst & 0xffffu) + 17u + ulen + sport + T.dst_port +
                      ulen + t0 + t1 + t2 + t3;
        // from byte 48 to the end of the row's last header piece: the tunnel header's last two bytes,
        // the options, then inner bytes; halfword k of that stream sits at row byte 50 + 2 k
        const uint32_t rb = tid * IP;
        const uint8_t *og = GENEVE && ol ? b.opt + (size_t)i * b.opt_stride : nullptr;
        auto half = [&](uint32_t k) -> uint32_t {       // payload halfword k (little-endian)
            const uint32_t o = 2u * k;
            if (GENEVE && o < ol) {
                const uint32_t w = *reinterpret_cast<const uint32_t *>(og + (o & ~3u));
                return (w >> (8u * (o & 2u))) & 0xffffu;
            }
            return tun_ld32(in32, rb + o - ol) & 0xffffu;
        };
        const uint32_t qend = 4u * ((50u + ol) >> 4) + 4u;
        uint32_t lo = tun_sw16(t3);
        for (uint32_t q = 12, k = 0; q < qend; q++, k += 2) {
            const uint32_t hi = half(k);
            h[q] = lo | (hi << 16);
            lo = half(k + 1);
        }
        if (CSUM) {
            for (uint32_t o = 0; o < ol; o += 2) hs += tun_sw16(half(o >> 1));
            m_sum[tid] = hs;
        }
    }
    __syncthreads();
    // ---- the UDP checksum: 8 lanes per frame over the staged inner bytes (len <= S here)
    if (CSUM) {
        const uint32_t g = tid & 7u;
        for (uint32_t r = tid >> 3; r < (uint32_t)R; r += TUN_NT / 8) {
            const bool on = r < nb && m_ovh[r] != 0u;
            uint32_t s = on ? tun_sum8(in32, r * IP, r * IP + m_len[r], g) : 0u;
            s = tun_group_sum(s);
            if (on && g == 0u) {
                uint32_t c = ~tun_fold(m_sum[r] + tun_sw16(tun_fold(s))) & 0xffffu;
                if (!c) c = 0xffffu;                    // RFC 768: a computed zero is transmitted as all ones
                hd32[(size_t)r * (HP / 4u) + 10] |= tun_sw16(c);
            }
        }
        __syncthreads();
    }
    // ---- the rows out: header pieces from their LDS image, the rest shifted out of the input rows
    const uint32_t per = out_stride / 16u;
    for (uint32_t k = tid; k < nb * per; k += TUN_NT) {
        const uint32_t r = k / per, p = k - r * per;
        const uint32_t ovh = m_ovh[r];
        if (!ovh) continue;
        const uint32_t len = m_len[r], cap = S < len ? S : len;
        const uint32_t W = ovh + cap < out_stride ? ovh + cap : out_stride;
        if (16u * p >= W) continue;
        uint4 v;
        if (p <= (ovh >> 4)) v = reinterpret_cast<const uint4 *>(hd32)[(size_t)r * (HP / 16u) + p];
        else v = tun_ld128h(in32, r * IP + 16u * p - ovh);
        tun_store_piece(out + (size_t)(b0 + r) * out_stride + 16u * p, v, W - 16u * p, true);
    }
}

// The select column from the records of a classify call (gf_tunnel_select).
__global__ __launch_bounds__(BLOCK) void k_tun_select(const uint8_t *recs, uint32_t kind, uint32_t n, uint32_t encap_ifindex,
                                                      uint8_t *select) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint8_t *r = recs + (size_t)i * 24;
    bool s;
    if (kind == GF_REC_EGRESS) s = (*reinterpret_cast<const uint16_t *>(r + 14) & GF_EG_F_ENCAP) != 0;   // eg_flags
    else s = encap_ifindex && r[1] == TC_REDIRECT &&                                                     // action, ifindex_lo
             *reinterpret_cast<const uint16_t *>(r + 8) == (uint16_t)encap_ifindex;
    select[i] = s ? 1 : 0;
}

template <bool GENEVE, int R>
__global__ __launch_bounds__(TUN_NT) void k_tun_decap(gf_frames fr, TunDev T, gf_tunnel_rx_out o) {
    extern __shared__ __attribute__((aligned(16))) uint4 tun_lds[];
    const uint32_t S = fr.snap_stride, P = tun_rx_pitch(S);
    uint32_t *in32 = reinterpret_cast<uint32_t *>(tun_lds);
    uint8_t *in8 = reinterpret_cast<uint8_t *>(tun_lds);
    uint32_t *m_st = in32 + (size_t)R * P / 4, *m_off = m_st + R, *m_len = m_off + R, *m_l4 = m_len + R;
    const uint32_t tid = threadIdx.x;
    const uint32_t b0 = blockIdx.x * R;
    const uint32_t nb = fr.n - b0 < (uint32_t)R ? fr.n - b0 : (uint32_t)R;
    {
        const uint8_t *src = fr.snap + (size_t)b0 * S;
        if (T.vec_in) {
            const uint32_t per = S / 16u;
            for (uint32_t k = tid; k < nb * per; k += TUN_NT) {
                const uint32_t r = k / per, j = k - r * per;
                tun_lds[(size_t)r * (P / 16u) + j] = reinterpret_cast<const uint4 *>(src)[k];
            }
        } else {
            for (uint32_t k = tid; k < nb * S; k += TUN_NT) {
                const uint32_t r = k / S, j = k - r * S;
                in8[(size_t)r * P + j] = src[k];
            }
        }
    }
    __syncthreads();
    // ---- one lane per frame: the outer headers (the order of include/gpuflow.h)
    uint32_t vni = 0, saddr = 0, ol = 0;
    if (tid < nb) {
        const uint32_t len = fr.len[b0 + tid], cap = S < len ? S : len;
        const uint32_t rb = tid * P;
        auto b8 = [&](uint32_t off) { return tun_ld32(in32, rb + off) & 0xffu; };
        auto be16 = [&](uint32_t off) { return tun_sw16(tun_ld32(in32, rb + off) & 0xffffu); };
        uint32_t st = GF_TUN_ST_OK, l4 = 0, off = 0;
        bool verify = false;
        do {
            if (cap < 14u) { st = GF_TUN_ST_BAD_OUTER; break; }
            if (be16(12) != 0x0800u) { st = GF_TUN_ST_NOT_TUNNEL; break; }
            if (cap < 34u) { st = GF_TUN_ST_BAD_OUTER; break; }
            const uint32_t vi = b8(14), fo = be16(20);
            const uint32_t daddr = __builtin_bswap32(tun_ld32(in32, rb + 30));
            if (b8(23) != 17u || (fo & 0x3fffu) || (T.local_ip && daddr != T.local_ip)) { st = GF_TUN_ST_NOT_TUNNEL; break; }
            const uint32_t ihl = vi & 15u;
            if ((vi >> 4) != 4u || ihl < 5u) { st = GF_TUN_ST_BAD_OUTER; break; }
            l4 = 14u + 4u * ihl;
            if (l4 + 8u > cap) { st = GF_TUN_ST_BAD_OUTER; break; }
            if (be16(l4 + 2) != T.dst_port) { st = GF_TUN_ST_NOT_TUNNEL; break; }
            if (be16(16) != len - 14u || be16(l4 + 4) != len - l4 || l4 + 16u > cap) { st = GF_TUN_ST_BAD_OUTER; break; }
            uint32_t s = 0;                             // RFC 791: the header's words sum to 0xffff
            for (uint32_t k = 14; k < l4; k += 4) { const uint32_t w = tun_ld32(in32, rb + k); s += (w & 0xffffu) + (w >> 16); }
            if (tun_fold(s) != 0xffffu) { st = GF_TUN_ST_BAD_OUTER; break; }
            const uint32_t w0 = tun_ld32(in32, rb + l4 + 8), w1 = tun_ld32(in32, rb + l4 + 12);
            if (!GENEVE) {                              // RFC 7348 section 5: flags 0x08, 24 + 8 reserved bits
                if (w0 != 0x08u || (w1 >> 24)) { st = GF_TUN_ST_BAD_HDR; break; }
            } else {                                    // RFC 8926 section 3.4
                ol = (w0 & 0x3fu) << 2;
                if ((w0 & 0xc0u) || (w0 & 0x4000u) || (w0 >> 16) != 0x5865u || l4 + 16u + ol > cap) { st = GF_TUN_ST_BAD_HDR; break; }
            }
            vni = __builtin_bswap32(w1) >> 8;
            saddr = __builtin_bswap32(tun_ld32(in32, rb + 26));
            off = l4 + 16u + ol;
            if (be16(l4 + 6)) {
                if (len <= S) verify = true;
                else st = GF_TUN_ST_OK_UNVERIFIED;
            }
        } while (false);
        m_st[tid] = st | (verify ? 0x100u : 0u);
        m_off[tid] = off; m_len[tid] = len; m_l4[tid] = l4;
    }
    __syncthreads();
    // ---- RFC 768: pseudo-header + datagram sum to 0xffff; 8 lanes per frame
    {
        const uint32_t g = tid & 7u;
        for (uint32_t r = tid >> 3; r < (uint32_t)R; r += TUN_NT / 8) {
            const bool on = r < nb && (m_st[r] & 0x100u);
            uint32_t s = 0;
            if (on) {
                s = tun_sum8(in32, r * P + m_l4[r], r * P + m_len[r], g);
                if (g == 0u) {
                    const uint32_t a = tun_ld32(in32, r * P + 26), d = tun_ld32(in32, r * P + 30);
                    s += (a & 0xffffu) + (a >> 16) + (d & 0xffffu) + (d >> 16) + 0x1100u + tun_sw16(m_len[r] - m_l4[r]);
                }
            }
            s = tun_group_sum(s);
            if (on && g == 0u) m_st[r] = tun_fold(s) == 0xffffu ? GF_TUN_ST_OK : GF_TUN_ST_BAD_CSUM;
        }
    }
    __syncthreads();
    // ---- the columns, by the frame's lane
    if (tid < nb) {
        const uint32_t i = b0 + tid, st = m_st[tid];
        const bool ok = st == GF_TUN_ST_OK || st == GF_TUN_ST_OK_UNVERIFIED;
        o.status[i] = (uint8_t)st;
        o.inner_len[i] = ok ? m_len[tid] - m_off[tid] : 0u;
        if (ok) {
            o.tunnel_id[i] = vni;
            o.outer_saddr[i] = saddr;
            if (o.opt_len) o.opt_len[i] = (uint8_t)ol;
            if (GENEVE) {
                const uint32_t nw = (ol < o.opt_stride ? ol : o.opt_stride) >> 2;
                uint32_t *d = reinterpret_cast<uint32_t *>(o.opt + (size_t)i * o.opt_stride);
                for (uint32_t k = 0; k < nw; k++) d[k] = tun_ld32(in32, tid * P + m_off[tid] - ol + 4u * k);
            }
        }
    }
    // ---- the inner rows
    const uint32_t IS = o.inner_stride, per = (IS + 15u) / 16u;
    for (uint32_t k = tid; k < nb * per; k += TUN_NT) {
        const uint32_t r = k / per, p = k - r * per;
        const uint32_t st = m_st[r];
        if (st != GF_TUN_ST_OK && st != GF_TUN_ST_OK_UNVERIFIED) continue;
        const uint32_t len = m_len[r], off = m_off[r], cap = S < len ? S : len;
        uint32_t W = cap - off;                         // inner bytes inside the snap (== inner_len when len <= S)
        if (W > IS) W = IS;
        if (16u * p >= W) continue;
        const uint4 v = tun_ld128h(in32, r * P + off + 16u * p);
        tun_store_piece(o.inner + (size_t)(b0 + r) * IS + 16u * p, v, W - 16u * p, T.vec_out != 0u);
    }
}

// ---------------------------------------------------------------- host
namespace {
TunDev tun_dev(const gf_tunnel_cfg &c) {
    TunDev T{};
    T.flags = c.flags; T.local_ip = c.local_ip; T.dst_port = c.dst_port;
    T.sport_min = c.sport_min; T.sport_span = (uint32_t)c.sport_max - c.sport_min;
    T.ttl = c.ttl; T.tos = c.tos;
    memcpy(T.smac, c.src_mac, 6);
    memcpy(T.dmac, c.dst_mac, 6);
    return T;
}
int tun_opts_check(const uint8_t *opt, uint32_t stride) {
    if (stride < 4 || stride > 64 || stride % 4 || ((uintptr_t)opt & 3u)) return -EINVAL;
    return 0;
}
}  // namespace

extern "C" {

int gf_tunnel_load(const gf_tunnel_cfg *cfg) {
    std::unique_lock<std::shared_mutex> g(prog_lock());
    if (!cfg) return -EFAULT;
    if (cfg->mode > GF_TUN_GENEVE || (cfg->flags & ~(GF_TUN_F_UDP_CSUM | GF_TUN_F_DF)) || !cfg->dst_port ||
        cfg->sport_min > cfg->sport_max)
        return -EINVAL;
    auto p = std::make_shared<ProgTunnel>();
    p->cfg = *cfg;
    return new_handle(p);
}

int gf_tunnel_encap(int tun, const gf_tunnel_tx *b, uint8_t *out, uint32_t out_stride, uint32_t *out_len,
                    uint8_t *status, void *stream) {
    std::shared_lock<std::shared_mutex> g(prog_lock());
    auto p = get_as<ProgTunnel>(tun);
    if (!p) return -EBADF;
    if (!b) return -EFAULT;
    const gf_frames &fr = b->frames;
    if (fr.n == 0) return 0;
    const bool geneve = p->cfg.mode == GF_TUN_GENEVE;
    if (!fr.snap || !fr.len || !b->remote_ip || !b->tunnel_id || !out || !out_len || !status) return -EFAULT;
    if (geneve && b->opt && !b->opt_len) return -EFAULT;
    if (fr.snap_stride < 14 || fr.snap_stride > 256) return -EINVAL;
    if (out_stride % 16 || out_stride < 128 || out_stride > 512 || ((uintptr_t)out & 15u) || out == fr.snap) return -EINVAL;
    if (geneve && b->opt && tun_opts_check(b->opt, b->opt_stride)) return -EINVAL;
    if (fr.n > (1u << 30)) return -E2BIG;
    hipStream_t s = (hipStream_t)stream;
    TunDev T = tun_dev(p->cfg);
    T.vec_in = (fr.snap_stride % 16 == 0) && ((uintptr_t)fr.snap & 15u) == 0;
    gf_tunnel_tx tx = *b;
    if (!geneve) { tx.opt = nullptr; tx.opt_len = nullptr; tx.opt_stride = 0; }
    const bool csum = p->cfg.flags & GF_TUN_F_UDP_CSUM;
    // rows per block by stride class: at most 40,464 B (39.5 KiB) of LDS a block (Geneve at stride 128)
    const uint32_t ip = tun_in_pitch(fr.snap_stride), hp = geneve ? 144u : 80u;
    const uint32_t R = fr.snap_stride <= 128 ? 128u : 64u;
    const size_t lds = (size_t)R * (ip + hp + 12) + 16;
    const uint32_t grid = (fr.n + R - 1) / R;
    ProfScope ps("k_tun_encap", s);
#define TUN_ENC(G, C, RR) hipLaunchKernelGGL((k_tun_encap<G, C, RR>), dim3(grid), dim3(TUN_NT), lds, s, tx, T, out, out_stride, out_len, status)
    if (R == 128) {
        if (geneve) { if (csum) TUN_ENC(true, true, 128); else TUN_ENC(true, false, 128); }
        else { if (csum) TUN_ENC(false, true, 128); else TUN_ENC(false, false, 128); }
    } else {
        if (geneve) { if (csum) TUN_ENC(true, true, 64); else TUN_ENC(true, false, 64); }
        else { if (csum) TUN_ENC(false, true, 64); else TUN_ENC(false, false, 64); }
    }
#undef TUN_ENC
    return hip_ok(hipGetLastError(), "k_tun_encap");
}

int gf_tunnel_select(const void *records, uint32_t rec_kind, uint32_t n, uint8_t *select, void *stream) {
    if (rec_kind != GF_REC_EGRESS && rec_kind != GF_REC_PIPELINE) return -EINVAL;
    if (n == 0) return 0;
    if (!records || !select) return -EFAULT;
    if (n > (1u << 30)) return -E2BIG;
    uint32_t ifx;
    {
        std::shared_lock<std::shared_mutex> g(prog_lock());
        ifx = node_cfg().encap_ifindex;
    }
    ProfScope ps("k_tun_select", (hipStream_t)stream);
    hipLaunchKernelGGL(k_tun_select, dim3((n + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, (hipStream_t)stream,
                       (const uint8_t *)records, rec_kind, n, ifx, select);
    return hip_ok(hipGetLastError(), "k_tun_select");
}

int gf_tunnel_decap(int tun, const gf_frames *outer, const gf_tunnel_rx_out *out, void *stream) {
    std::shared_lock<std::shared_mutex> g(prog_lock());
    auto p = get_as<ProgTunnel>(tun);
    if (!p) return -EBADF;
    if (!outer || !out) return -EFAULT;
    const gf_frames &fr = *outer;
    if (fr.n == 0) return 0;
    const bool geneve = p->cfg.mode == GF_TUN_GENEVE;
    if (!fr.snap || !fr.len || !out->inner || !out->inner_len || !out->tunnel_id || !out->outer_saddr || !out->status)
        return -EFAULT;
    if (geneve && (!out->opt || !out->opt_len)) return -EFAULT;
    if (fr.snap_stride < 64 || fr.snap_stride > 512) return -EINVAL;
    if (out->inner_stride < 14 || out->inner_stride > 256 || out->inner == fr.snap) return -EINVAL;
    if (geneve && tun_opts_check(out->opt, out->opt_stride)) return -EINVAL;
    if (fr.n > (1u << 30)) return -E2BIG;
    hipStream_t s = (hipStream_t)stream;
    TunDev T = tun_dev(p->cfg);
    T.vec_in = (fr.snap_stride % 16 == 0) && ((uintptr_t)fr.snap & 15u) == 0;
    T.vec_out = (out->inner_stride % 16 == 0) && ((uintptr_t)out->inner & 15u) == 0;
    const uint32_t R = fr.snap_stride <= 256 ? 128u : 64u;   // <= 36 KiB of LDS a block
    const size_t lds = (size_t)R * (tun_rx_pitch(fr.snap_stride) + 16) + 32;
    const uint32_t grid = (fr.n + R - 1) / R;
    ProfScope ps("k_tun_decap", s);
#define TUN_DEC(G, RR) hipLaunchKernelGGL((k_tun_decap<G, RR>), dim3(grid), dim3(TUN_NT), lds, s, fr, T, *out)
    if (R == 128) { if (geneve) TUN_DEC(true, 128); else TUN_DEC(false, 128); }
    else { if (geneve) TUN_DEC(true, 64); else TUN_DEC(false, 64); }
#undef TUN_DEC
    return hip_ok(hipGetLastError(), "k_tun_decap");
}

}  // extern "C"
