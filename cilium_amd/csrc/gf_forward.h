// gf_forward.h — forwarding the verdicts: gf_forward_load / gf_forward_queues / gf_forward_frames
// (included at the end of gf_kernels.hip, after gf_xdp_frames.h: its tile size, and the wave
// scans of gf_events.h).
//
// In the reference a verdict moves the packet: TC_ACT_SHOT frees the skb, TC_ACT_OK hands it to
// the stack, redirect(ifindex) puts it on that device's queue.  Here that is a stable multi-way
// partition of the batch's rows into at most GF_FWD_MAX_QUEUES queues, in two calls:
//   k_fwd_queues     one record per lane: the queue byte by the rule of include/gpuflow.h, from
//                    two to four bytes of the record and the 64 KB ifindex_lo -> queue table
//   k_fwd_count      one tile of FWD_TILE consecutive frames per block: the tile's rows per
//                    queue, into a workspace laid out [queue][tile], and as row n_queues the
//                    queue bytes that name no queue (counts[3])
//   k_fwd_scan       one block, as k_xdpf_scan: one linear exclusive prefix over the
//                    (n_queues + 1) * tiles words, in place.  That is the first output row of
//                    every (queue, tile) pair, and qoff[q] as the base of (q, tile 0)
//   k_fwd_scatter    one block per tile: every lane's rank among the lanes of its queue, then the
//                    forwarded rows copied piece by piece by consecutive lanes; len and index by
//                    the row's lane
// No block waits for another, and no output position comes from an atomic: the order inside a
// queue is the arrival order.
//
// A lane's rank in its queue, in a wave: the lanes with an equal queue id from six ballots over
// the id's bits (fwd_peers), and the popcount below the lane.  Across the tile's waves: s_cnt
// [wave][queue], the lowest lane of each set storing the set's size, then one lane per queue
// turning its column into an exclusive prefix.  LDS banks: 32-bit reads and writes bank by
// (address / 4) mod 32 within each half of the wave, so a row of 64 words puts queues q and
// q + 32 on one bank: a wave's stores and loads of its own row are 2-way at worst, and only when
// both queues occur in one half; the column pass (lane q, lanes q and q + 32 in different
// halves) is conflict-free.
#pragma once

#define FWD_TILE XDPF_TILE
#define FWD_WAVES (FWD_TILE / 64)

// The lanes of the wave that are forwarded and hold this lane's queue id (q < 64).  Every lane of
// the wave calls it; the result means something in the forwarded lanes only.
__device__ __forceinline__ uint64_t fwd_peers(uint32_t q, bool fwd) {
    uint64_t m = __ballot(fwd);
#pragma unroll
    for (uint32_t b = 0; b < 6u; b++) {
        const bool bit = (q >> b) & 1u;
        const uint64_t bb = __ballot(bit);
        m &= bit ? bb : ~bb;
    }
    return m;
}

// kind: GF_REC_EGRESS / GF_REC_PIPELINE (24 B: stage 0, action 1, flags 4, ifindex_lo 8, eg_flags 14)
// or GF_REC_LB (12 B: action 0).
__global__ __launch_bounds__(BLOCK) void k_fwd_queues(const uint8_t *recs, uint32_t kind, uint32_t n, const uint8_t *table,
                                                      uint32_t stack_q, uint32_t resp_q, uint32_t def_q, uint8_t *queue) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    uint32_t act, q;
    bool xdp = false, resp = false;
    const uint8_t *r = recs + (size_t)i * (kind == GF_REC_LB ? 12u : 24u);
    if (kind == GF_REC_LB) {
        act = r[0];
    } else {
        act = r[1];
        if (kind == GF_REC_EGRESS)
            resp = (*reinterpret_cast<const uint16_t *>(r + 14) & (GF_EG_F_ARP | GF_EG_F_RESPONDER | GF_EG_F_ICMP6_TE)) != 0;
        else {
            xdp = r[0] == GF_STAGE_XDP;
            resp = (r[4] & (GF_PIPE_F_ICMP6_TE | GF_PIPE_F_RESPONDER)) != 0;
        }
    }
    if (xdp) q = GF_FWD_DROP;
    else if (resp) q = resp_q;
    else if (act == TC_SHOT) q = GF_FWD_DROP;
    else if (act == TC_OK) q = stack_q;
    else if (act == TC_REDIRECT) q = kind == GF_REC_LB ? def_q : table[*reinterpret_cast<const uint16_t *>(r + 8)];
    else q = GF_FWD_DROP;
    queue[i] = (uint8_t)q;
}

// ws: [nq + 1][nt] words; block t writes column t.
__global__ __launch_bounds__(FWD_TILE) void k_fwd_count(const uint8_t *queue, uint32_t n, uint32_t nq, uint32_t nt,
                                                        uint32_t *ws) {
    __shared__ uint32_t s_cnt[FWD_WAVES][64];
    __shared__ uint32_t s_inv[FWD_WAVES];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
    s_cnt[wv][lane] = 0u;                               // the wave's own row: its stores below follow in order
    const uint32_t i = blockIdx.x * FWD_TILE + tid;
    const uint32_t q = i < n ? queue[i] : GF_FWD_DROP;
    const bool fwd = q < nq;
    const uint64_t peers = fwd_peers(q, fwd);
    const uint64_t inv = __ballot(!fwd && q != GF_FWD_DROP);
    if (fwd && (peers & ((1ull << lane) - 1ull)) == 0) s_cnt[wv][q] = (uint32_t)__popcll(peers);
    if (lane == 0) s_inv[wv] = (uint32_t)__popcll(inv);
    __syncthreads();
    if (tid <= nq) {
        uint32_t c = 0;
#pragma unroll
        for (int k = 0; k < FWD_WAVES; k++) c += tid < nq ? s_cnt[k][tid] : s_inv[k];
        ws[(size_t)tid * nt + blockIdx.x] = c;
    }
}

// One block, as k_xdpf_scan, over the W = (nq + 1) * nt words of ws: lane k takes the run
// [k * per, (k + 1) * per).  The run that holds word q * nt writes qoff[q] (q <= nq: qoff[nq], the
// base of the row of the queue bytes that name no queue, is the number of forwarded rows).
__global__ __launch_bounds__(1024) void k_fwd_scan(uint32_t *ws, uint32_t nt, uint32_t nq, uint32_t n, uint32_t max_out,
                                                   uint32_t *qoff, uint32_t *counts) {
    __shared__ uint32_t wm[1024 / 64];
    __shared__ uint32_t s_fwd;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
    const uint32_t W = (nq + 1u) * nt;
    const uint32_t per = (W + 1023u) / 1024u;
    const uint32_t lo = tid * per < W ? tid * per : W, hi = lo + per < W ? lo + per : W;
    uint32_t m = 0, j = lo;
    for (; j + 8u <= hi; j += 8u) {                     // eight loads in flight: a lane's run is 65 words at 1M frames and 64 queues
        uint32_t v[8];
#pragma unroll
        for (int k = 0; k < 8; k++) v[k] = ws[j + k];
#pragma unroll
        for (int k = 0; k < 8; k++) m += v[k];
    }
    for (; j < hi; j++) m += ws[j];
    const uint32_t im = evd_wave_scan(m, lane);
    if (lane == 63u) wm[wv] = im;
    __syncthreads();
    uint32_t pm = im - m, all = 0;
    for (uint32_t k = 0; k < 1024 / 64; k++) {
        if (k < wv) pm += wm[k];
        all += wm[k];
    }
    uint32_t qn = (lo + nt - 1u) / nt, nb = qn * nt;    // the next row start at or past lo
    const auto put = [&](uint32_t at, uint32_t e) {
        if (at == nb) {
            qoff[qn] = pm;
            if (qn == nq) s_fwd = pm;
            qn++; nb += nt;
        }
        ws[at] = pm;
        pm += e;
    };
    for (j = lo; j + 8u <= hi; j += 8u) {
        uint32_t v[8];
#pragma unroll
        for (int k = 0; k < 8; k++) v[k] = ws[j + k];
#pragma unroll
        for (int k = 0; k < 8; k++) put(j + k, v[k]);
    }
    for (; j < hi; j++) put(j, ws[j]);
    __syncthreads();
    if (tid == 0) {
        const uint32_t f = s_fwd;
        counts[0] = f; counts[1] = n - f; counts[2] = f < max_out ? f : max_out; counts[3] = all - f;
    }
}

// PIECE, pps: as k_xdpf_scatter.  The tile's forwarded rows take the places [0, m) in queue
// order, arrival order inside a queue: consecutive lanes copy consecutive pieces of that list, so
// a source row is read and a destination row written as one run, and the rows of one queue land
// one behind the other.
template <uint32_t PIECE>
__global__ __launch_bounds__(FWD_TILE) void k_fwd_scatter(gf_frames fr, const uint8_t *queue, uint32_t nq, uint32_t nt,
                                                          const uint32_t *ws, uint8_t *snap, uint32_t *len, uint32_t *index,
                                                          uint32_t max_out, uint32_t pps) {
    __shared__ uint32_t s_cnt[FWD_WAVES][64];
    __shared__ uint32_t s_base[64], s_loc[64];          // per queue: the first output row of (q, tile); its first place in the tile
    __shared__ uint32_t s_dst[FWD_TILE];                // by place: the output row, ~0 = past the capacity
    __shared__ uint16_t s_src[FWD_TILE];                // by place: the row's lane
    __shared__ uint32_t s_m;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
    if (ws[blockIdx.x] >= max_out) return;              // block-uniform: (0, tile) has the tile's lowest base
    s_cnt[wv][lane] = 0u;
    const uint32_t i0 = blockIdx.x * FWD_TILE, i = i0 + tid;
    const uint32_t q = i < fr.n ? queue[i] : GF_FWD_DROP;
    const bool fwd = q < nq;
    const uint64_t peers = fwd_peers(q, fwd);
    const uint32_t below = (uint32_t)__popcll(peers & ((1ull << lane) - 1ull));
    if (fwd && below == 0) s_cnt[wv][q] = (uint32_t)__popcll(peers);
    __syncthreads();
    if (tid < 64u) {                                    // lane q: the column of queue q, exclusive over the waves
        uint32_t v[FWD_WAVES], t = 0;
#pragma unroll
        for (int k = 0; k < FWD_WAVES; k++) v[k] = s_cnt[k][tid];
#pragma unroll
        for (int k = 0; k < FWD_WAVES; k++) { s_cnt[k][tid] = t; t += v[k]; }
        const uint32_t it = evd_wave_scan(t, lane);
        s_loc[tid] = it - t;
        s_base[tid] = tid < nq ? ws[(size_t)tid * nt + blockIdx.x] : 0u;
        if (tid == 63u) s_m = it;
    }
    __syncthreads();
    if (fwd) {
        const uint32_t w = s_cnt[wv][q] + below;
        const uint32_t dst = s_base[q] + w, place = s_loc[q] + w;
        const bool in = dst < max_out;
        s_src[place] = (uint16_t)tid;
        s_dst[place] = in ? dst : ~0u;
        if (in) {
            len[dst] = fr.len[i];
            if (index) index[dst] = i;
        }
    }
    __syncthreads();
    const uint32_t m = s_m;
    const uint8_t *in = fr.snap + (size_t)i0 * fr.snap_stride;
    for (uint32_t k = tid; k < m * pps; k += FWD_TILE) {
        const uint32_t p = k / pps, po = (k - p * pps) * PIECE;
        const uint32_t dr = s_dst[p];
        if (dr == ~0u) continue;
        const uint8_t *s = in + (size_t)s_src[p] * fr.snap_stride + po;
        uint8_t *d = snap + (size_t)dr * fr.snap_stride + po;
        if (PIECE == 16u) *reinterpret_cast<uint4 *>(d) = *reinterpret_cast<const uint4 *>(s);
        else if (PIECE == 4u) *reinterpret_cast<uint32_t *>(d) = *reinterpret_cast<const uint32_t *>(s);
        else *d = *s;
    }
}

// ---------------------------------------------------------------- host
namespace {
struct FwdWs { DevBuf buf; };                           // (n_queues + 1) * tiles words
FwdWs &fwd_ws() { static const char tag = 0; return cur_ctx().get<FwdWs>(&tag); }
bool fwd_queue_ok(uint32_t q, uint32_t nq) { return q < nq || q == GF_FWD_DROP; }
}  // namespace

extern "C" {

int gf_forward_load(const gf_forward_cfg *cfg) {
    if (!cfg) return -EFAULT;
    if (cfg->n_ifindex && !cfg->ifindex) return -EFAULT;
    const uint32_t nq = cfg->n_queues;
    if (nq < 1 || nq > GF_FWD_MAX_QUEUES) return -EINVAL;
    if (!fwd_queue_ok(cfg->stack_queue, nq) || !fwd_queue_ok(cfg->responder_queue, nq) || !fwd_queue_ok(cfg->default_queue, nq))
        return -EINVAL;
    for (uint32_t k = 0; k < cfg->n_ifindex; k++)
        if (!fwd_queue_ok(cfg->ifindex[k].queue, nq)) return -EINVAL;
    auto p = std::make_shared<Forward>();
    p->n_queues = nq;
    p->stack_queue = cfg->stack_queue; p->responder_queue = cfg->responder_queue; p->default_queue = cfg->default_queue;
    p->table.assign(65536, cfg->default_queue);
    for (uint32_t k = 0; k < cfg->n_ifindex; k++) p->table[cfg->ifindex[k].ifindex_lo] = cfg->ifindex[k].queue;
    return new_handle(p);
}

int gf_forward_queues(int fwd, const void *records, uint32_t rec_kind, uint32_t n, uint8_t *queue, void *stream) {
    std::shared_lock<std::shared_mutex> g(prog_lock());
    auto p = get_as<Forward>(fwd);
    if (!p) return -EBADF;
    if (n && (!records || !queue)) return -EFAULT;
    if (rec_kind != GF_REC_EGRESS && rec_kind != GF_REC_PIPELINE && rec_kind != GF_REC_LB) return -EINVAL;
    if (n > (1u << 30)) return -E2BIG;
    if (n == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    {
        std::lock_guard<std::mutex> fg(p->mu);
        if (!p->d_table.p) {                            // the handle's first call: the table, once
            int r;
            if ((r = p->d_table.ensure(65536))) return r;
            if (hip_ok(hipMemcpy(p->d_table.p, p->table.data(), 65536, hipMemcpyHostToDevice), "forward table")) {
                p->d_table.release();
                return -EIO;
            }
        }
    }
    ProfScope ps("k_fwd_queues", s);
    hipLaunchKernelGGL(k_fwd_queues, dim3((n + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, s, (const uint8_t *)records, rec_kind, n,
                       (const uint8_t *)p->d_table.p, (uint32_t)p->stack_queue, (uint32_t)p->responder_queue,
                       (uint32_t)p->default_queue, queue);
    return hip_ok(hipGetLastError(), "k_fwd_queues");
}

int gf_forward_frames(const gf_frames *frames, const uint8_t *queue, uint32_t n_queues, const gf_forward_out *out,
                      void *stream) {
    if (!frames || !queue || !out || !out->qoff || !out->counts) return -EFAULT;
    const gf_frames &fr = *frames;
    const uint32_t n = fr.n, nq = n_queues;
    if (n && (!fr.snap || !fr.len)) return -EFAULT;
    if (out->snap && !out->len) return -EFAULT;
    if (nq < 1 || nq > GF_FWD_MAX_QUEUES) return -EINVAL;
    if (n && (fr.snap_stride < 14 || fr.snap_stride > 256)) return -EINVAL;   // a header snap, as on every frame entry point
    if (!out->snap && (out->len || out->index)) return -EINVAL;
    {
        // no in-place mode: no output buffer may share a byte with the frames, their lengths or the queue column
        const uint64_t cap = out->snap ? out->max_out : 0u;
        const void *ob[5] = {out->snap, out->len, out->index, out->qoff, out->counts};
        const uint64_t on[5] = {cap * fr.snap_stride, cap * 4u, cap * 4u, (nq + 1u) * 4u, 16u};
        for (int k = 0; k < 5; k++)
            if (xdpf_overlap(ob[k], on[k], fr.snap, (uint64_t)n * fr.snap_stride) ||
                xdpf_overlap(ob[k], on[k], fr.len, (uint64_t)n * 4u) || xdpf_overlap(ob[k], on[k], queue, n))
                return -EINVAL;
    }
    if (n > (1u << 30)) return -E2BIG;
    hipStream_t s = (hipStream_t)stream;
    int r;
    if (n == 0) {
        if ((r = hip_ok(hipMemsetAsync(out->qoff, 0, (nq + 1u) * 4u, s), "gf_forward_frames qoff"))) return r;
        return hip_ok(hipMemsetAsync(out->counts, 0, 16, s), "gf_forward_frames counts");
    }
    CtxScope cx(s);
    const uint32_t nt = (n + FWD_TILE - 1) / FWD_TILE;
    FwdWs &w = fwd_ws();
    const size_t want = (size_t)(nq + 1u) * nt * 4u;
    if (w.buf.bytes < want && (r = w.buf.ensure(want))) return r;
    uint32_t *ws = (uint32_t *)w.buf.p;
    {
        ProfScope ps("k_fwd_count", s);
        hipLaunchKernelGGL(k_fwd_count, dim3(nt), dim3(FWD_TILE), 0, s, queue, n, nq, nt, ws);
        if ((r = hip_ok(hipGetLastError(), "k_fwd_count"))) return r;
    }
    {
        ProfScope ps("k_fwd_scan", s);
        hipLaunchKernelGGL(k_fwd_scan, dim3(1), dim3(1024), 0, s, ws, nt, nq, n, out->snap ? out->max_out : 0u, out->qoff,
                           out->counts);
        if ((r = hip_ok(hipGetLastError(), "k_fwd_scan"))) return r;
    }
    if (!out->snap || !out->max_out) return 0;
    ProfScope ps("k_fwd_scatter", s);
    const uintptr_t al = (uintptr_t)fr.snap | (uintptr_t)out->snap | fr.snap_stride;
#define FWD_SCATTER(P) hipLaunchKernelGGL(k_fwd_scatter<P>, dim3(nt), dim3(FWD_TILE), 0, s, fr, queue, nq, nt, \
                                          (const uint32_t *)ws, out->snap, out->len, out->index, out->max_out,  \
                                          fr.snap_stride / P)
    if (!(al & 15u)) FWD_SCATTER(16u);
    else if (!(al & 3u)) FWD_SCATTER(4u);
    else FWD_SCATTER(1u);
#undef FWD_SCATTER
    return hip_ok(hipGetLastError(), "k_fwd_scatter");
}

}  // extern "C"
