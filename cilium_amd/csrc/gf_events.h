// gf_events.h — draining the event ring on the device with cilium monitor's filters
// (included at the end of gf_kernels.hip: kernels and the host side of
// gf_event_filter_load / gf_event_drain).
//
// The rule is match() of cilium/cmd/monitor.go:144-156 over the source and destination its
// four handlers pass (monitor.go:165,182,199,215); include/gpuflow.h states it.  A drain is a
// stream compaction in three launches over blocks of EVD_NT records, one lane per record:
//   k_evd_count    the predicate from 8 bytes of each record (12 in packed mode); per block the
//                  matches per type, the unknown types and the output bytes (EvdBlk)
//   k_evd_scan     one block: the exclusive prefix of matches and bytes over the block sums, in
//                  place, and the totals (EvdHead)
//   k_evd_scatter  the predicate again, the rank of each match inside its block, and the copies
// No block waits for another (no decoupled look-back): a block that spins on a flag of a block
// that has not been scheduled hangs, and the two extra passes read 8 bytes of 160 per record.
// The count word is read by k_evd_count only, which saves it in the head, so the reset at the
// end of k_evd_scatter cannot be seen by a block of the same drain.
#pragma once

#define EVD_NT 256
#define EVF_WORDS 2048u                // one 65536-bit bitmap

struct EvfDev {
    const uint32_t *from, *to, *rel;   // bitmaps; null: the flag was not given
    uint32_t type_mask;
};
struct EvdBlk {                        // per block of EVD_NT records; k_evd_scan turns m and bytes into exclusive prefixes
    uint32_t m, unk, t[4];
    uint64_t bytes;
};
struct EvdHead {
    gf_event_drain_out tot;            // tot.count by k_evd_count, the rest by k_evd_scan (written, bytes: when nothing is cut)
    uint32_t cut, pad;                 // the matches take more than out_bytes
};
struct EvdArgs {
    gf_event_ring ring;
    EvfDev F;
    uint32_t first, max_n;             // max_n: the effective window (never 0)
    uint64_t out_bytes;
};
struct EvdRec {
    uint32_t type;                     // 1..4; 0: unknown
    uint32_t match;
    uint32_t wire, len;                // bytes copied from the slot, bytes taken in out (a match only)
};

__device__ __forceinline__ bool evf_has(const uint32_t *bm, uint32_t id) { return (bm[id >> 5] >> (id & 31u)) & 1u; }

// [lo, hi) of the drain's window, from the count word as k_evd_count found it
__device__ __forceinline__ uint64_t evd_window_end(const EvdArgs &A, uint32_t count) {
    const uint64_t avail = count < A.ring.capacity ? count : A.ring.capacity;
    const uint64_t end = (uint64_t)A.first + A.max_n;
    return avail < end ? avail : end;
}

template <bool PACKED>
__device__ __forceinline__ EvdRec evd_eval(const uint8_t *rec, const EvfDev &F) {
    const uint32_t *w = reinterpret_cast<const uint32_t *>(rec);
    const uint32_t h = w[0], t = h & 0xffu, src = h >> 16;
    EvdRec r{};
    if (t - 1u > 3u) return r;
    r.type = t;
    // drop: uint16(dn.DstID), the u32 at byte 24; trace: the u16 there; debug, capture: 0
    const uint32_t dst = (t == 1u || t == 4u) ? (w[6] & 0xffffu) : 0u;
    if (F.type_mask && !((F.type_mask >> t) & 1u)) return r;
    if (F.from && !evf_has(F.from, src)) return r;
    if (F.to && !evf_has(F.to, dst)) return r;
    if (F.rel && !evf_has(F.rel, src) && !evf_has(F.rel, dst)) return r;
    r.match = 1;
    r.wire = r.len = GF_EVENT_RECORD;
    if (PACKED) {
        uint32_t cap = t == 2u ? 0u : w[3];
        if (cap > GF_EVENT_RECORD) cap = GF_EVENT_RECORD;
        uint32_t wl = (t == 2u ? 20u : t == 3u ? 24u : 32u) + cap;
        if (wl > GF_EVENT_RECORD) wl = GF_EVENT_RECORD;
        r.wire = wl;
        r.len = (wl + 7u) & ~7u;
    }
    return r;
}

__device__ __forceinline__ uint32_t evd_wave_sum(uint32_t v) {
    for (int d = 32; d >= 1; d >>= 1) v += (uint32_t)__shfl_xor((int)v, d);
    return v;
}
__device__ __forceinline__ uint32_t evd_wave_max(uint32_t v) {
    for (int d = 32; d >= 1; d >>= 1) { const uint32_t o = (uint32_t)__shfl_xor((int)v, d); v = o > v ? o : v; }
    return v;
}
// inclusive prefix sums inside a wave
__device__ __forceinline__ uint32_t evd_wave_scan(uint32_t v, uint32_t lane) {
    for (uint32_t d = 1; d < 64u; d <<= 1) { const uint32_t u = (uint32_t)__shfl_up((int)v, d); if (lane >= d) v += u; }
    return v;
}
__device__ __forceinline__ unsigned long long evd_wave_scan64(unsigned long long v, uint32_t lane) {
    for (uint32_t d = 1; d < 64u; d <<= 1) { const unsigned long long u = __shfl_up(v, d); if (lane >= d) v += u; }
    return v;
}

template <bool PACKED>
__global__ __launch_bounds__(EVD_NT) void k_evd_count(EvdArgs A, EvdHead *head, EvdBlk *blk) {
    __shared__ uint32_t bins[6];                        // matches of type 1..4, unknown types, bytes
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    if (tid < 6u) bins[tid] = 0u;
    const uint32_t count = *A.ring.count;
    if (blockIdx.x == 0 && tid == 0) head->tot.count = count;
    const uint64_t hi = evd_window_end(A, count);
    const uint64_t i = (uint64_t)A.first + (uint64_t)blockIdx.x * EVD_NT + tid;
    const bool in = i < hi;
    EvdRec r{};
    if (in) r = evd_eval<PACKED>(A.ring.records + i * GF_EVENT_RECORD, A.F);
    __syncthreads();
    for (uint32_t t = 1; t <= 4u; t++) {
        const uint64_t b = __ballot(r.match && r.type == t);
        if (lane == 0 && b) atomicAdd(&bins[t - 1u], (uint32_t)__popcll(b));
    }
    const uint64_t ub = __ballot(in && !r.type);
    const uint32_t by = evd_wave_sum(r.match ? r.len : 0u);
    if (lane == 0) {
        if (ub) atomicAdd(&bins[4], (uint32_t)__popcll(ub));
        if (by) atomicAdd(&bins[5], by);
    }
    __syncthreads();
    if (tid == 0) {
        EvdBlk o;
        o.m = bins[0] + bins[1] + bins[2] + bins[3];
        o.unk = bins[4];
        for (int t = 0; t < 4; t++) o.t[t] = bins[t];
        o.bytes = bins[5];
        blk[blockIdx.x] = o;
    }
}

#define EVD_SCAN_NT 1024
// One block: lane k takes the run of block sums [k * per, (k + 1) * per), so the scan over the
// lanes' totals spans 16 waves whatever nb is.
__global__ __launch_bounds__(EVD_SCAN_NT) void k_evd_scan(EvdArgs A, EvdHead *head, EvdBlk *blk, uint32_t nb) {
    __shared__ uint32_t wm[EVD_SCAN_NT / 64];
    __shared__ unsigned long long wb[EVD_SCAN_NT / 64];
    __shared__ uint32_t tot[5];                         // matches of type 1..4, unknown types
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
    if (tid < 5u) tot[tid] = 0u;
    const uint32_t per = (nb + EVD_SCAN_NT - 1) / EVD_SCAN_NT;
    const uint32_t lo = tid * per < nb ? tid * per : nb, hi = lo + per < nb ? lo + per : nb;
    uint32_t m = 0, c[5] = {0, 0, 0, 0, 0};
    unsigned long long by = 0;
    for (uint32_t j = lo; j < hi; j++) {
        const EvdBlk e = blk[j];
        m += e.m; by += e.bytes; c[4] += e.unk;
        for (int t = 0; t < 4; t++) c[t] += e.t[t];
    }
    const uint32_t im = evd_wave_scan(m, lane);
    const unsigned long long ib = evd_wave_scan64(by, lane);
    if (lane == 63u) { wm[wv] = im; wb[wv] = ib; }
    __syncthreads();
    for (int t = 0; t < 5; t++) {
        const uint32_t s = evd_wave_sum(c[t]);
        if (lane == 0 && s) atomicAdd(&tot[t], s);
    }
    uint32_t pm = im - m, all_m = 0;
    unsigned long long pb = ib - by, all_b = 0;
    for (uint32_t k = 0; k < EVD_SCAN_NT / 64; k++) {
        if (k < wv) { pm += wm[k]; pb += wb[k]; }
        all_m += wm[k]; all_b += wb[k];
    }
    for (uint32_t j = lo; j < hi; j++) {
        const uint32_t em = blk[j].m;
        const unsigned long long eb = blk[j].bytes;
        blk[j].m = pm; blk[j].bytes = pb;
        pm += em; pb += eb;
    }
    __syncthreads();
    if (tid == 0) {
        const uint32_t count = head->tot.count, cap = A.ring.capacity;
        const uint64_t end = evd_window_end(A, count);
        gf_event_drain_out o{};
        o.count = count;
        o.lost = (count > cap ? count : cap) - cap;
        o.seen = end > A.first ? (uint32_t)(end - A.first) : 0u;
        o.matched = all_m;
        o.unknown = tot[4];
        for (int t = 0; t < 4; t++) o.by_type[t + 1] = tot[t];
        o.written = all_m;
        o.bytes = all_b;
        head->tot = o;
        head->cut = all_b > A.out_bytes ? 1u : 0u;
    }
}

// PACKED: wire lengths, pieces of 8 bytes; slots otherwise, pieces of 16 bytes when VEC.  VEC: the
// ring's records and out are aligned to the piece, so every piece moves as one load and one store.
template <bool PACKED, bool VEC>
__global__ __launch_bounds__(EVD_NT) void k_evd_scatter(EvdArgs A, uint32_t flags, uint8_t *out, uint32_t *out_off,
                                                        gf_event_drain_out *res, const EvdHead *head, const EvdBlk *blk) {
    constexpr uint32_t PIECE = (!PACKED && VEC) ? 16u : 8u, PPS = GF_EVENT_RECORD / PIECE;
    __shared__ uint32_t s_off[EVD_NT];                  // by rank: the record's offset from the block's first output byte
    __shared__ uint8_t s_src[EVD_NT], s_len[EVD_NT], s_wire[EVD_NT];
    __shared__ uint32_t wm[EVD_NT / 64], wb[EVD_NT / 64], s_nfit, s_end;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
    if (tid == 0) { s_nfit = 0u; s_end = 0u; }
    const uint64_t hi = evd_window_end(A, head->tot.count);
    const uint64_t i0 = (uint64_t)A.first + (uint64_t)blockIdx.x * EVD_NT;
    EvdRec r{};
    if (i0 + tid < hi) r = evd_eval<PACKED>(A.ring.records + (i0 + tid) * GF_EVENT_RECORD, A.F);
    const uint64_t bal = __ballot(r.match);
    const uint32_t by = r.match ? r.len : 0u, iby = evd_wave_scan(by, lane);
    if (lane == 63u) { wm[wv] = (uint32_t)__popcll(bal); wb[wv] = iby; }
    __syncthreads();
    uint32_t rank = (uint32_t)__popcll(bal & ((1ull << lane) - 1ull)), off = iby - by;
    for (uint32_t k = 0; k < wv; k++) { rank += wm[k]; off += wb[k]; }
    const uint32_t base_m = blk[blockIdx.x].m;
    const uint64_t base_b = blk[blockIdx.x].bytes;
    // the records are stored while the running total fits: the stored ones are a prefix of the ranks
    const bool fit = r.match && base_b + off + r.len <= A.out_bytes;
    if (fit) {
        s_off[rank] = off; s_src[rank] = (uint8_t)tid; s_len[rank] = (uint8_t)r.len; s_wire[rank] = (uint8_t)r.wire;
        if (out_off) out_off[base_m + rank] = (uint32_t)(base_b + off);
    }
    const uint64_t fb = __ballot(fit);
    const uint32_t fe = evd_wave_max(fit ? off + r.len : 0u);
    if (lane == 0 && fb) { atomicAdd(&s_nfit, (uint32_t)__popcll(fb)); atomicMax(&s_end, fe); }
    __syncthreads();
    const uint32_t nfit = s_nfit;
    for (uint32_t k = tid; k < nfit * PPS; k += EVD_NT) {
        const uint32_t q = k / PPS, po = (k - q * PPS) * PIECE;
        if (po >= s_len[q]) continue;
        const uint8_t *src = A.ring.records + (i0 + s_src[q]) * GF_EVENT_RECORD + po;
        uint8_t *dst = out + base_b + s_off[q] + po;
        const uint32_t nv = s_wire[q] - po < PIECE ? s_wire[q] - po : PIECE;   // the rest of the piece is padding: zeros
        if (PIECE == 16u) {
            *reinterpret_cast<uint4 *>(dst) = *reinterpret_cast<const uint4 *>(src);
        } else if (VEC) {
            uint2 v = *reinterpret_cast<const uint2 *>(src);
            if (nv < 8u) {
                const unsigned long long keep = (1ull << (8u * nv)) - 1ull;
                v.x &= (uint32_t)keep; v.y &= (uint32_t)(keep >> 32);
            }
            *reinterpret_cast<uint2 *>(dst) = v;
        } else {
            for (uint32_t j = 0; j < 8u; j++) dst[j] = j < nv ? src[j] : (uint8_t)0;
        }
    }
    if (tid != 0) return;
    // where the output is cut, the block in which the running total passes out_bytes has the two figures
    const uint32_t cut = head->cut;
    const uint32_t bb = wb[0] + wb[1] + wb[2] + wb[3];
    if (cut && base_b <= A.out_bytes && base_b + bb > A.out_bytes) {
        res->written = base_m + nfit;
        res->bytes = base_b + s_end;
        if (out_off) out_off[base_m + nfit] = (uint32_t)(base_b + s_end);
    }
    if (blockIdx.x == 0) {
        const gf_event_drain_out t = head->tot;
        res->count = t.count; res->lost = t.lost; res->seen = t.seen; res->matched = t.matched;
        res->unknown = t.unknown; res->pad = 0u;
        for (int k = 0; k < 5; k++) res->by_type[k] = t.by_type[k];
        if (!cut) {
            res->written = t.written; res->bytes = t.bytes;
            if (out_off) out_off[t.written] = (uint32_t)t.bytes;
        }
        if (flags & GF_EVD_F_RESET) *A.ring.count = 0u;
    }
}

// ---------------------------------------------------------------- host
namespace {
struct EvdWs { DevBuf buf; };                           // EvdHead, then one EvdBlk per block
EvdWs &evd_ws() { static const char tag = 0; return cur_ctx().get<EvdWs>(&tag); }
}  // namespace

extern "C" {

int gf_event_filter_load(const gf_event_filter_cfg *cfg) {
    if (!cfg) return -EFAULT;
    const uint16_t *list[3] = {cfg->from, cfg->to, cfg->related};
    const uint32_t n[3] = {cfg->n_from, cfg->n_to, cfg->n_related};
    for (int k = 0; k < 3; k++) if (n[k] && !list[k]) return -EFAULT;
    if (cfg->type_mask & ~0x1eu) return -EINVAL;
    for (int k = 0; k < 3; k++) if (n[k] > GF_EVF_MAX_IDS) return -E2BIG;
    auto p = std::make_shared<EventFilter>();
    p->type_mask = cfg->type_mask;
    p->bits.assign(3 * EVF_WORDS, 0u);
    for (int k = 0; k < 3; k++) {
        p->given[k] = n[k] != 0;
        for (uint32_t j = 0; j < n[k]; j++) p->bits[k * EVF_WORDS + (list[k][j] >> 5)] |= 1u << (list[k][j] & 31u);
    }
    return new_handle(p);
}

int gf_event_drain(int filter, const gf_event_ring *ring, uint32_t first, uint32_t max_n, uint32_t flags,
                   uint8_t *out, uint64_t out_bytes, uint32_t *out_off, gf_event_drain_out *res, void *stream) {
    std::shared_lock<std::shared_mutex> g(prog_lock());
    auto p = get_as<EventFilter>(filter);
    if (!p) return -EBADF;
    if (!ring || !ring->records || !ring->count || !res) return -EFAULT;
    if (!out && out_bytes) return -EFAULT;
    if (flags & ~(GF_EVD_F_PACKED | GF_EVD_F_RESET)) return -EINVAL;
    const uintptr_t r0 = (uintptr_t)ring->records, r1 = r0 + (uint64_t)ring->capacity * GF_EVENT_RECORD;
    if (out_bytes && (uintptr_t)out < r1 && r0 < (uintptr_t)out + out_bytes) return -EINVAL;
    if (r0 & 3u) return -EINVAL;
    if (max_n > GF_EVD_MAX_WINDOW) return -E2BIG;
    hipStream_t s = (hipStream_t)stream;
    CtxScope cx(s);
    CallOrder co(s, std::vector<OrderPt *>{});          // with the ring of gf_set_event_ring: this call's turn at it
    int r;
    {
        std::lock_guard<std::mutex> fg(p->mu);
        if (!p->d_bits.p) {                             // the handle's first drain: the bitmaps, once
            if ((r = p->d_bits.ensure(3 * EVF_WORDS * 4))) return r;
            if (hip_ok(hipMemcpy(p->d_bits.p, p->bits.data(), 3 * EVF_WORDS * 4, hipMemcpyHostToDevice), "event filter")) {
                p->d_bits.release();
                return -EIO;
            }
        }
    }
    EvdArgs A{};
    A.ring = *ring;
    const uint32_t *bm = (const uint32_t *)p->d_bits.p;
    A.F = EvfDev{p->given[0] ? bm : nullptr, p->given[1] ? bm + EVF_WORDS : nullptr,
                 p->given[2] ? bm + 2 * EVF_WORDS : nullptr, p->type_mask};
    A.first = first;
    A.max_n = max_n ? max_n : GF_EVD_MAX_WINDOW;
    A.out_bytes = out_bytes;
    // the grid covers what the window can be at most; blocks past *ring->count find nothing
    const uint32_t room = first < ring->capacity ? ring->capacity - first : 0u;
    const uint32_t wmax = room < A.max_n ? room : A.max_n;
    const uint32_t nb = wmax ? (wmax + EVD_NT - 1) / EVD_NT : 1u;
    EvdWs &w = evd_ws();
    const size_t want = sizeof(EvdHead) + (size_t)nb * sizeof(EvdBlk);
    if (w.buf.bytes < want && (r = w.buf.ensure(want))) return r;
    EvdHead *head = (EvdHead *)w.buf.p;
    EvdBlk *blk = (EvdBlk *)(head + 1);
    const bool packed = flags & GF_EVD_F_PACKED;
    const uintptr_t al = r0 | (uintptr_t)out;
    const bool vec = packed ? (al & 7u) == 0 : (al & 15u) == 0;
    {
        ProfScope ps("k_evd_count", s);
        if (packed) hipLaunchKernelGGL(k_evd_count<true>, dim3(nb), dim3(EVD_NT), 0, s, A, head, blk);
        else hipLaunchKernelGGL(k_evd_count<false>, dim3(nb), dim3(EVD_NT), 0, s, A, head, blk);
    }
    {
        ProfScope ps("k_evd_scan", s);
        hipLaunchKernelGGL(k_evd_scan, dim3(1), dim3(EVD_SCAN_NT), 0, s, A, head, blk, nb);
    }
    {
        ProfScope ps("k_evd_scatter", s);
#define EVD_SCATTER(P, V) hipLaunchKernelGGL((k_evd_scatter<P, V>), dim3(nb), dim3(EVD_NT), 0, s, A, flags, out, out_off, res, \
                                             (const EvdHead *)head, (const EvdBlk *)blk)
        if (packed) { if (vec) EVD_SCATTER(true, true); else EVD_SCATTER(true, false); }
        else { if (vec) EVD_SCATTER(false, true); else EVD_SCATTER(false, false); }
#undef EVD_SCATTER
    }
    return hip_ok(hipGetLastError(), "gf_event_drain");
}

}  // extern "C"
