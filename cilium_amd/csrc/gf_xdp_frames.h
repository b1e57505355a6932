// gf_xdp_frames.h — the prefilter over raw frames: gf_xdp_filter_frames (included at the end of
// gf_kernels.hip, after gf_events.h, whose wave scans it uses).
//
// bpf_xdp.o on --prefilter-device (bpf/bpf_xdp.c:158-184) is the one program that removes
// traffic: XDP_DROP frames reach nothing behind it.  The call is that on a batch: the verdict of
// every frame, and the XDP_PASS frames packed in arrival order with their lengths and batch
// indices, as a gf_frames the next entry point takes.  A stable stream compaction in three
// launches over tiles of XDPF_TILE consecutive frames:
//   k_xdpf_verdict   one frame per lane: ethertype and the two addresses from the row (FrameA),
//                    xdp_verdict with k_xdp_lds's LDS staging when the tables fit; the verdict
//                    byte, the tile's pass count, the stats sums
//   k_xdpf_scan      one block: the exclusive prefix of the pass counts, in place, and counts[]
//   k_xdpf_scatter   one block per tile: ranks from the verdict bytes, then the passing rows
//                    copied piece by piece by consecutive lanes; len and index by the row's lane
// No block waits for another, as in gf_event_drain.
#pragma once

#define XDPF_TILE 1024

// LDS: the block stages the root summary, the /32 set and the endpoint set exactly as k_xdp_lds
// does and takes its IPv4 path; otherwise every frame takes xdp_verdict over HBM / L2.  The
// IPv4 body below is k_xdp_lds's, restated over FrameA: sharing it through a device function
// would have to leave that kernel's registers and scratch as they are, which is not given.
template <bool LDS>
__global__ __launch_bounds__(XDPF_TILE) void k_xdpf_verdict(gf_frames fr, XdpDev x, XdpLds L, uint8_t *verdict,
                                                            uint32_t *tile_cnt, unsigned long long *stats) {
    extern __shared__ uint4 xl[];
    __shared__ uint32_t sl[272];
    __shared__ uint32_t s_wc[2][XDPF_TILE / 64];          // the waves' pass counts, by the parity of the block's trip
    Stats st{sl};
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
    const uint64_t *rs = reinterpret_cast<const uint64_t *>(xl);
    const uint32_t h4b = L.h4set ? 4u << L.h4bits : L.h4_bytes, lxb = L.lxset ? 4u << L.lxbits : L.lxc_bytes;
    const uint8_t *h4s = reinterpret_cast<const uint8_t *>(xl) + GF_TRIE_RSUM_BYTES;
    const uint8_t *lxs = h4s + h4b;
    if (LDS) {
        uint4 *d = xl;
        const uint4 *src = reinterpret_cast<const uint4 *>(x.l4.rsum);
        for (uint32_t k = tid; k < GF_TRIE_RSUM_BYTES / 16; k += XDPF_TILE) d[k] = src[k];
        d += GF_TRIE_RSUM_BYTES / 16;
        src = reinterpret_cast<const uint4 *>(L.h4set ? (const void *)L.h4set : (const void *)x.h4.slots);
        for (uint32_t k = tid; k < h4b / 16; k += XDPF_TILE) d[k] = src[k];
        d += h4b / 16;
        src = reinterpret_cast<const uint4 *>(L.lxset ? (const void *)L.lxset : (const void *)x.lxc.slots);
        for (uint32_t k = tid; k < lxb / 16; k += XDPF_TILE) d[k] = src[k];
    }
    if (stats) st.init(); else __syncthreads();
    const bool al = ((reinterpret_cast<uintptr_t>(fr.snap) | fr.snap_stride) & 3u) == 0;
    const bool w4 = al && fr.snap_stride >= 36u, w6 = al && fr.snap_stride >= 56u;
    const uint32_t nt = (fr.n + XDPF_TILE - 1) / XDPF_TILE;
    uint32_t n_drop = 0, n_pass = 0, s_len = 0, s_ab = 0;      // the lane's counter sums, reduced once at the end
    uint32_t par = 0;
    for (uint32_t t = blockIdx.x; t < nt; t += gridDim.x, par ^= 1u) {      // block-uniform trips
        const uint32_t i = t * XDPF_TILE + tid;
        uint8_t v = 0;
        if (i < fr.n) {
            const uint32_t len = fr.len[i];
            uint32_t ab = 1;                               // output record
            const FrameA a{fr.snap + (size_t)i * fr.snap_stride, fr.snap_stride < len ? fr.snap_stride : len, w4, w6};
            const uint32_t et = a.et(len);
            if (!LDS || et != 0x0800 || len < 34) {
                v = xdp_verdict(x, a, len, et, ab);
            } else {
                const uint32_t sa = a.saddr4();
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
                    const uint32_t lk[5] = {a.daddr4(), 0, 0, 0, 1u};
                    const bool ep = L.lxset ? aset_has(reinterpret_cast<const uint32_t *>(lxs), L.lxbits, L.lxzero, lk[0])
                                  : L.lxc_bytes ? lds_has<20>(lxs, x.lxc.mask, x.lxc.slot_size, lk, key_hash<20>(lk))
                                                : ht_find<20>(x.lxc, lk, key_hash<20>(lk)) >= 0;
                    v = ep ? XDP_PASS_ : XDP_DROP_;
                }
            }
            verdict[i] = v;
            n_drop += v == XDP_DROP_; n_pass += v == XDP_PASS_; s_len += len; s_ab += ab;
        }
        // The tile's pass count.  Trip k fills s_wc[k & 1] before its barrier and lane 0 reads it
        // after; the waves fill that half again in trip k + 2, behind the barrier of trip k + 1,
        // which lane 0 reaches only after this read: one barrier a tile.
        const uint64_t pb = __ballot(v == XDP_PASS_);
        if (lane == 0) s_wc[par][wv] = (uint32_t)__popcll(pb);
        __syncthreads();
        if (tid == 0) {
            uint32_t c = 0;
#pragma unroll
            for (int k = 0; k < XDPF_TILE / 64; k++) c += s_wc[par][k];
            tile_cnt[t] = c;
        }
    }
    if (stats) {
        st.xdp_sums(n_drop, n_pass, s_len, s_ab);
        st.flush(stats);
    }
}

// One block, as k_evd_scan: lane k takes the run of tiles [k * per, (k + 1) * per), so the scan
// over the lanes' totals spans 16 waves whatever nt is (up to 2^20 tiles: 1024 a lane).
// counts: [0] passed, [1] dropped, [2] written, [3] 0.
__global__ __launch_bounds__(1024) void k_xdpf_scan(uint32_t *tile_cnt, uint32_t nt, uint32_t n, uint32_t max_out,
                                                    uint32_t *counts) {
    __shared__ uint32_t wm[1024 / 64];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
    const uint32_t per = (nt + 1023u) / 1024u;
    const uint32_t lo = tid * per < nt ? tid * per : nt, hi = lo + per < nt ? lo + per : nt;
    uint32_t m = 0;
    for (uint32_t j = lo; j < hi; j++) m += tile_cnt[j];
    const uint32_t im = evd_wave_scan(m, lane);
    if (lane == 63u) wm[wv] = im;
    __syncthreads();
    uint32_t pm = im - m, all = 0;
    for (uint32_t k = 0; k < 1024 / 64; k++) {
        if (k < wv) pm += wm[k];
        all += wm[k];
    }
    for (uint32_t j = lo; j < hi; j++) {
        const uint32_t e = tile_cnt[j];
        tile_cnt[j] = pm;
        pm += e;
    }
    if (tid == 0) {
        counts[0] = all; counts[1] = n - all; counts[2] = all < max_out ? all : max_out; counts[3] = 0u;
    }
}

// PIECE: the bytes one lane moves at a time: 16 when the rows of both buffers are 16-byte
// aligned, 4 when they are 4-byte aligned, else 1.  pps: pieces per row (snap_stride / PIECE).
template <uint32_t PIECE>
__global__ __launch_bounds__(XDPF_TILE) void k_xdpf_scatter(gf_frames fr, const uint8_t *verdict, const uint32_t *tile_off,
                                                            uint8_t *snap, uint32_t *len, uint32_t *index,
                                                            uint32_t max_out, uint32_t pps) {
    __shared__ uint16_t s_src[XDPF_TILE];               // by rank in the tile: the row's lane
    __shared__ uint32_t s_wc[XDPF_TILE / 64];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
    const uint32_t base = tile_off[blockIdx.x];
    if (base >= max_out) return;                        // block-uniform: every row of the tile ranks past the capacity
    const uint32_t i0 = blockIdx.x * XDPF_TILE, i = i0 + tid;
    const bool pass = i < fr.n && verdict[i] == XDP_PASS_;
    const uint64_t pb = __ballot(pass);
    if (lane == 0) s_wc[wv] = (uint32_t)__popcll(pb);
    __syncthreads();
    uint32_t rank = (uint32_t)__popcll(pb & ((1ull << lane) - 1ull)), m = 0;
    for (uint32_t k = 0; k < XDPF_TILE / 64; k++) {
        if (k < wv) rank += s_wc[k];
        m += s_wc[k];
    }
    const uint32_t room = max_out - base;
    if (m > room) m = room;                             // the rows written: a prefix of the tile's ranks
    if (pass && rank < m) {
        s_src[rank] = (uint16_t)tid;
        len[base + rank] = fr.len[i];
        if (index) index[base + rank] = i;
    }
    __syncthreads();
    const uint8_t *in = fr.snap + (size_t)i0 * fr.snap_stride;
    uint8_t *out = snap + (size_t)base * fr.snap_stride;
    for (uint32_t k = tid; k < m * pps; k += XDPF_TILE) {
        const uint32_t q = k / pps, po = (k - q * pps) * PIECE;
        const uint8_t *s = in + (size_t)s_src[q] * fr.snap_stride + po;
        uint8_t *d = out + (size_t)k * PIECE;           // == q * snap_stride + po: the output is one run
        if (PIECE == 16u) *reinterpret_cast<uint4 *>(d) = *reinterpret_cast<const uint4 *>(s);
        else if (PIECE == 4u) *reinterpret_cast<uint32_t *>(d) = *reinterpret_cast<const uint32_t *>(s);
        else *d = *s;
    }
}

// ---------------------------------------------------------------- host
namespace {
// gf_xdp_classify's rule for k_xdp_lds, for k_xdpf_verdict<true> (the same staging under the same
// budget, GF_XDP_LDS_KB included): fills L and the dynamic LDS size, false = the HBM kernel.
bool xdpf_lds_plan(const XdpDev &x, XdpLds &L, uint32_t &lds) {
    static const bool no_lds = getenv("GF_XDP_NOLDS") != nullptr;
    if (no_lds || !x.l4.rsum || !x.has_h4 || x.l4.addr_bytes != 4) return false;
    static const uint32_t cap = getenv("GF_XDP_LDS_KB") ? 1024u * (uint32_t)atoi(getenv("GF_XDP_LDS_KB")) : 48u * 1024u;
    L.h4set = x.h4set; L.h4bits = x.h4bits; L.h4zero = x.h4zero;
    L.lxset = x.lxset; L.lxbits = x.lxbits; L.lxzero = x.lxzero;
    const uint64_t hb = (uint64_t)(x.h4.mask + 1) * x.h4.slot_size, lb = (uint64_t)(x.lxc.mask + 1) * x.lxc.slot_size;
    if (!L.h4set && x.h4.slots && x.h4.ksz == 8 && hb % 16 == 0 && GF_TRIE_RSUM_BYTES + hb <= std::min(cap, 96u * 1024u))
        L.h4_bytes = (uint32_t)hb;
    const uint32_t h4b = L.h4set ? 4u << L.h4bits : L.h4_bytes;
    if (!L.lxset && x.lxc.slots && x.lxc.ksz == 20 && lb % 16 == 0 && GF_TRIE_RSUM_BYTES + h4b + lb <= cap)
        L.lxc_bytes = (uint32_t)lb;
    lds = GF_TRIE_RSUM_BYTES + h4b + (L.lxset ? 4u << L.lxbits : L.lxc_bytes);
    if (lds > std::max(cap, (uint32_t)GF_TRIE_RSUM_BYTES)) return false;
    static std::atomic<uint32_t> lds_set{0};
    if (lds > lds_set.load()) {
        if (hipFuncSetAttribute((const void *)k_xdpf_verdict<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) !=
            hipSuccess) {
            (void)hipGetLastError();
            return false;
        }
        uint32_t cur = lds_set.load();
        while (lds > cur && !lds_set.compare_exchange_weak(cur, lds)) {}
    }
    return true;
}
bool xdpf_overlap(const void *a, uint64_t an, const void *b, uint64_t bn) {
    return a && b && an && bn && (uintptr_t)a < (uintptr_t)b + bn && (uintptr_t)b < (uintptr_t)a + an;
}
}  // namespace

extern "C" {

int gf_xdp_filter_frames(int prog, const gf_frames *frames, const gf_xdp_frames_out *out, void *stream) {
    std::shared_lock<std::shared_mutex> g(prog_lock());
    auto p = get_as<ProgXdp>(prog);
    if (!p) return -EBADF;
    if (!frames || !out || !out->counts) return -EFAULT;
    const gf_frames &fr = *frames;
    const uint32_t n = fr.n;
    if (n && (!fr.snap || !fr.len)) return -EFAULT;
    if (out->snap && !out->len) return -EFAULT;
    if (n && (fr.snap_stride < 14 || fr.snap_stride > 256)) return -EINVAL;   // a header snap, as on every frame entry point
    if (!out->snap && (out->len || out->index)) return -EINVAL;
    {
        // no in-place mode: no output buffer may share a byte with the frames or their lengths
        const uint64_t cap = out->snap ? out->max_out : 0u;
        const void *ob[5] = {out->verdict, out->snap, out->len, out->index, out->counts};
        const uint64_t on[5] = {n, cap * fr.snap_stride, cap * 4u, cap * 4u, 16u};
        for (int k = 0; k < 5; k++)
            if (xdpf_overlap(ob[k], on[k], fr.snap, (uint64_t)n * fr.snap_stride) || xdpf_overlap(ob[k], on[k], fr.len, (uint64_t)n * 4u))
                return -EINVAL;
    }
    if (n > (1u << 30)) return -E2BIG;
    hipStream_t s = (hipStream_t)stream;
    if (n == 0) return hip_ok(hipMemsetAsync(out->counts, 0, 16, s), "gf_xdp_filter_frames counts");
    CtxScope cx(s);
    std::lock_guard<std::mutex> wg(p->ff_mu);
    MapLocks ML;
    lock_xdp_maps(ML, *p);
    ML.lock();
    CallOrder co(s, ML);
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
    // the workspace: one word per tile, then the verdict bytes when the caller takes none
    const uint32_t nt = (n + XDPF_TILE - 1) / XDPF_TILE;
    const size_t voff = ((size_t)nt * 4 + 15) & ~(size_t)15;
    const size_t want = voff + (out->verdict ? 0 : n);
    if (p->ff_ws.bytes < want && (r = p->ff_ws.ensure(want))) return r;
    uint32_t *tile = (uint32_t *)p->ff_ws.p;
    uint8_t *verdict = out->verdict ? out->verdict : (uint8_t *)p->ff_ws.p + voff;
    const uint32_t cap = stream_grid_cap();
    {
        XdpLds L{};
        uint32_t lds = 0;
        const bool in_lds = xdpf_lds_plan(x, L, lds);
        ProfScope ps(in_lds ? "k_xdpf_verdict_lds" : "k_xdpf_verdict", s);     // the profiler tells the two apart
        if (in_lds) {
            uint32_t grid = std::min<uint32_t>(resident_blocks(lds <= 78u * 1024u ? 2u : 1u), nt);
            if (cap && grid > cap) grid = cap;
            hipLaunchKernelGGL(k_xdpf_verdict<true>, dim3(grid), dim3(XDPF_TILE), lds, s, fr, x, L, verdict, tile,
                               (unsigned long long *)stats_sink());
        } else {
            hipLaunchKernelGGL(k_xdpf_verdict<false>, dim3(stream_grid(n, XDPF_TILE)), dim3(XDPF_TILE), 0, s, fr, x, L,
                               verdict, tile, (unsigned long long *)stats_sink());
        }
        if ((r = hip_ok(hipGetLastError(), "k_xdpf_verdict"))) return r;
    }
    {
        ProfScope ps("k_xdpf_scan", s);
        hipLaunchKernelGGL(k_xdpf_scan, dim3(1), dim3(1024), 0, s, tile, nt, n, out->snap ? out->max_out : 0u, out->counts);
        if ((r = hip_ok(hipGetLastError(), "k_xdpf_scan"))) return r;
    }
    if (!out->snap || !out->max_out) return 0;
    ProfScope ps("k_xdpf_scatter", s);
    const uintptr_t al = (uintptr_t)fr.snap | (uintptr_t)out->snap | fr.snap_stride;
#define XDPF_SCATTER(P) hipLaunchKernelGGL(k_xdpf_scatter<P>, dim3(nt), dim3(XDPF_TILE), 0, s, fr, (const uint8_t *)verdict, \
                                           (const uint32_t *)tile, out->snap, out->len, out->index, out->max_out,           \
                                           fr.snap_stride / P)
    if (!(al & 15u)) XDPF_SCATTER(16u);
    else if (!(al & 3u)) XDPF_SCATTER(4u);
    else XDPF_SCATTER(1u);
#undef XDPF_SCATTER
    return hip_ok(hipGetLastError(), "k_xdpf_scatter");
}

}  // extern "C"
