// gf_map_bulk.h — the device paths of the map API (gf_maps.cpp calls in through namespace gf,
// gf_internal.h): the bulk insert of gf_map_update_batch (k_bulk_hash, _dups, _probe, _insert)
// and the chunked dump of gf_map_lookup_batch (k_dump_gather) (included by gf_kernels.hip after
// gf_host_entry.h; it leans on none of the stages before it, only on gf_internal.h's host objects
// and gf_device.h's probes).

// ================================================================ bulk insert (gf_map_update_batch)
// A batch of distinct keys loaded straight into a fixed-capacity table in HBM:
// one lane per element walks the key's probe sequence, overwrites the key's slot
// (BPF_ANY) or claims the first EMPTY slot with a CAS on its state word (BUSY),
// fills key and value and publishes FULL with a release store; readers acquire
// the state word first.  Keys are distinct (checked first), so the outcome is
// that of the sequential updates.
__device__ __forceinline__ void bulk_key_words(const uint8_t *k, uint32_t ksz, uint32_t *kw) {
    for (int q = 0; q < 16; q++) kw[q] = 0;
    for (uint32_t b = 0; b < ksz; b++) kw[b >> 2] |= (uint32_t)k[b] << (8 * (b & 3));
}
__device__ __forceinline__ bool bulk_eq(const uint8_t *a, const uint8_t *b, uint32_t n) {
    for (uint32_t q = 0; q < n; q++) if (a[q] != b[q]) return false;
    return true;
}
__global__ __launch_bounds__(BLOCK) void k_bulk_hash(const uint8_t *keys, uint32_t ksz, uint32_t mode, uint32_t n, uint32_t *h) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        uint32_t kw[16];
        bulk_key_words(keys + (size_t)i * ksz, ksz, kw);
        h[i] = gf_key_hash(kw, ksz, mode);
    }
}
// flag[0]: two equal keys in the batch (equal keys have equal hashes: adjacent runs after the sort)
__global__ __launch_bounds__(BLOCK) void k_bulk_dups(const uint32_t *hs, const uint32_t *idx, const uint8_t *keys,
                                                     uint32_t ksz, uint32_t n, uint32_t *flag) {
    for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < n; j += gridDim.x * blockDim.x)
        for (int64_t k = (int64_t)j - 1; k >= 0 && hs[k] == hs[j]; k--)
            if (bulk_eq(keys + (size_t)idx[k] * ksz, keys + (size_t)idx[j] * ksz, ksz)) atomicOr(&flag[0], 1u);
}
__device__ __forceinline__ uint32_t bulk_state_word(const gf_htab_desc &d, uint64_t j) {
    const uint32_t *sw = reinterpret_cast<const uint32_t *>(d.slots + j * d.slot_size + (d.ksz & ~3u));
    return __hip_atomic_load(sw, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
}
// flag[1]: a key of the batch is already in the table
__global__ __launch_bounds__(BLOCK) void k_bulk_probe(gf_htab_desc d, const uint8_t *keys, const uint32_t *h, uint32_t n,
                                                      uint32_t *flag) {
    const uint32_t sb = 8 * (d.ksz & 3u);
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const uint8_t *k = keys + (size_t)i * d.ksz;
        uint64_t j = gf_home_slot(h[i], d.mask, d.slot_size);
        for (uint64_t p = 0; p <= d.mask; p++, j = (j + 1) & d.mask) {
            const uint32_t st = (bulk_state_word(d, j) >> sb) & 0xffu;
            if (st == GF_SLOT_EMPTY) break;
            if (st == GF_SLOT_FULL && bulk_eq(d.slots + j * d.slot_size, k, d.ksz)) { atomicOr(&flag[1], 1u); break; }
        }
    }
}
__global__ __launch_bounds__(BLOCK) void k_bulk_insert(gf_htab_desc d, uint32_t codec, const uint8_t *keys,
                                                       const uint8_t *vals, const uint32_t *h, uint32_t n) {
    const uint32_t sb = 8 * (d.ksz & 3u), kw0 = d.ksz & ~3u;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const uint8_t *k = keys + (size_t)i * d.ksz, *ext = vals + (size_t)i * d.vsz;
        uint8_t in[128];
        if (codec == GF_VCODEC_CT) gf_ct_encode(ext, in);
        else if (codec == GF_VCODEC_POL) gf_pol_encode(ext, in);
        else for (uint32_t b = 0; b < d.vsz; b++) in[b] = ext[b];
        uint32_t keep = 0;
        for (uint32_t b = kw0; b < d.ksz; b++) keep |= (uint32_t)k[b] << (8 * (b - kw0));
        auto put_val = [&](uint64_t j) {
            uint8_t *sl = d.slots + j * d.slot_size;
            for (uint32_t b = 0; b < d.vin; b++) sl[d.voff + b] = in[b];
            for (uint32_t b = d.vin; b < d.vsz; b++) d.vals[j * d.sstride + (b - d.vin)] = in[b];
        };
        uint64_t j = gf_home_slot(h[i], d.mask, d.slot_size);
        for (uint64_t p = 0; p <= d.mask;) {
            uint32_t *sw = reinterpret_cast<uint32_t *>(d.slots + j * d.slot_size + kw0);
            uint32_t w = bulk_state_word(d, j);
            const uint32_t st = (w >> sb) & 0xffu;
            if (st == GF_SLOT_FULL && bulk_eq(d.slots + j * d.slot_size, k, d.ksz)) { put_val(j); break; }
            if (st == GF_SLOT_EMPTY) {
                const uint32_t busy = keep | ((uint32_t)GF_SLOT_BUSY << sb);
                uint32_t seen = w;
                __hip_atomic_compare_exchange_strong(sw, &seen, busy, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                     __HIP_MEMORY_SCOPE_AGENT);
                if (seen != w) continue;                       // lost the slot: look at it again
                uint8_t *sl = d.slots + j * d.slot_size;
                for (uint32_t b = 0; b < kw0; b++) sl[b] = k[b];
                put_val(j);
                __hip_atomic_store(sw, keep | ((uint32_t)GF_SLOT_FULL << sb), __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
                atomicAdd(d.count, 1u);
                break;
            }
            p++;
            j = (j + 1) & d.mask;
        }
    }
}

namespace gf {
int dev_bulk_insert(Map &m, const uint8_t *keys, const uint8_t *vals, uint32_t n, uint64_t flags, bool &fallback) {
    fallback = true;
    int dc = 0;
    if (hipGetDeviceCount(&dc) != hipSuccess || dc == 0 || m.vsz > 128 || m.ksz > 64) return 0;
    const bool had = m.dev_auth();
    uint64_t before = 0;
    if (had) { uint32_t c; if (m.dev_count(c)) return 0; before = c; }
    if (before + n > dev_insert_limit(m)) return 0;     // the host path reports E2BIG at the exact element
    static std::mutex mu;
    std::lock_guard<std::mutex> lk(mu);
    static DevBuf dk, dv, dh, dhs, didx, tmp, dflag;
    auto grow = [](DevBuf &b, size_t want) -> int { return b.bytes >= want ? 0 : b.ensure(want); };
    int r;
    if ((r = grow(dk, (size_t)n * m.ksz)) || (r = grow(dv, (size_t)n * m.vsz)) || (r = grow(dh, (size_t)n * 4)) ||
        (r = grow(dhs, (size_t)n * 4)) || (r = grow(didx, (size_t)n * 4)) || (r = grow(dflag, 8)))
        return r;
    if (!had) {                                          // create the (empty) replica
        m.dev_valid = false;
        if ((r = m.push((hipStream_t)0))) return r;
    }
    const hipStream_t s = (hipStream_t)0;
    if (hip_ok(hipMemcpy(dk.p, keys, (size_t)n * m.ksz, hipMemcpyHostToDevice), "bulk keys") ||
        hip_ok(hipMemcpy(dv.p, vals, (size_t)n * m.vsz, hipMemcpyHostToDevice), "bulk vals") ||
        hip_ok(hipMemset(dflag.p, 0, 8), "bulk flags"))
        return -EIO;
    m.xfer_h2d += (size_t)n * (m.ksz + m.vsz);
    const gf_htab_desc d = m.hdesc();
    const uint32_t g = std::min<uint32_t>((n + BLOCK - 1) / BLOCK, 65535u);
    hipLaunchKernelGGL(k_bulk_hash, dim3(g), dim3(BLOCK), 0, s, (const uint8_t *)dk.p, m.ksz, m.ht.mode, n, (uint32_t *)dh.p);
    size_t tb = 0;
    (void)rocprim::radix_sort_pairs(nullptr, tb, (uint32_t *)dh.p, (uint32_t *)dhs.p, rocprim::counting_iterator<uint32_t>(0u),
                                    (uint32_t *)didx.p, n, 0, 32, s);
    if ((r = grow(tmp, tb + 256))) return r;
    tb = tmp.bytes;
    if (hip_ok(rocprim::radix_sort_pairs(tmp.p, tb, (uint32_t *)dh.p, (uint32_t *)dhs.p, rocprim::counting_iterator<uint32_t>(0u),
                                         (uint32_t *)didx.p, n, 0, 32, s), "bulk sort"))
        return -EIO;
    hipLaunchKernelGGL(k_bulk_dups, dim3(g), dim3(BLOCK), 0, s, (const uint32_t *)dhs.p, (const uint32_t *)didx.p,
                       (const uint8_t *)dk.p, m.ksz, n, (uint32_t *)dflag.p);
    if (had && flags == GF_NOEXIST)
        hipLaunchKernelGGL(k_bulk_probe, dim3(g), dim3(BLOCK), 0, s, d, (const uint8_t *)dk.p, (const uint32_t *)dh.p, n,
                           (uint32_t *)dflag.p);
    uint32_t fl[2] = {0, 0};
    if (hip_ok(hipGetLastError(), "bulk check") || hip_ok(hipMemcpy(fl, dflag.p, 8, hipMemcpyDeviceToHost), "bulk flags"))
        return -EIO;
    if (fl[0] || fl[1]) return 0;                        // duplicates / EEXIST: the sequential host path
    hipLaunchKernelGGL(k_bulk_insert, dim3(g), dim3(BLOCK), 0, s, d, m.ht.codec, (const uint8_t *)dk.p,
                       (const uint8_t *)dv.p, (const uint32_t *)dh.p, n);
    if (hip_ok(hipGetLastError(), "k_bulk_insert") || hip_ok(hipDeviceSynchronize(), "bulk sync")) return -EIO;
    m.host_valid = false;
    m.dev_gen++;
    m.dev_count_hi = before + n;
    m.ev_pending = 0;
    m.st_floor = m.lru_seq;
    fallback = false;
    return 0;
}
}  // namespace gf

// ================================================================ chunked dump (gf_map_lookup_batch)
// The FULL slots of a range of a device-authoritative hash map, compacted in
// slot order on the device (rocPRIM select over the slot indices), their keys
// and reference-layout values gathered into a staging buffer: only the entries
// cross PCIe, a 64M-entry CT dumps without its 16 GB slot arrays moving.
struct SlotFull {
    const uint8_t *slots;
    uint64_t base;
    uint32_t ss, ksz;
    __device__ bool operator()(uint32_t j) const { return slots[(base + j) * ss + ksz] == GF_SLOT_FULL; }
};
__global__ __launch_bounds__(BLOCK) void k_dump_gather(gf_htab_desc d, uint32_t codec, uint64_t base, const uint32_t *sel,
                                                       const uint32_t *nsel, uint32_t cap, uint8_t *keys, uint8_t *vals) {
    const uint32_t n = min(*nsel, cap);
    for (uint32_t t = blockIdx.x * blockDim.x + threadIdx.x; t < n; t += gridDim.x * blockDim.x) {
        const uint64_t i = base + sel[t];
        const uint8_t *sl = d.slots + i * d.slot_size;
        for (uint32_t b = 0; b < d.ksz; b++) keys[(size_t)t * d.ksz + b] = sl[b];
        uint8_t in[128], ext[128];
        for (uint32_t b = 0; b < d.vin; b++) in[b] = sl[d.voff + b];
        for (uint32_t b = d.vin; b < d.vsz; b++) in[b] = d.vals[i * d.sstride + (b - d.vin)];
        if (codec == GF_VCODEC_CT) gf_ct_decode(in, ext);
        else if (codec == GF_VCODEC_POL) gf_pol_decode(in, ext);
        else for (uint32_t b = 0; b < d.vsz; b++) ext[b] = in[b];
        for (uint32_t b = 0; b < d.vsz; b++) vals[(size_t)t * d.vsz + b] = ext[b];
    }
}

namespace gf {
int dev_dump(Map &m, uint64_t start, uint32_t max, uint8_t *keys, uint8_t *vals, uint32_t *n, uint64_t *next) {
    static std::mutex mu;                                // the staging buffers below
    std::lock_guard<std::mutex> g(mu);
    static DevBuf sel, nsel, tmp, dk, dv;
    *n = 0; *next = start;
    if (!max || start >= m.ht.nslots) { *next = m.ht.nslots; return 0; }
    if (m.vsz > 128) return -EOPNOTSUPP;
    const uint64_t R = std::min<uint64_t>(m.ht.nslots - start, std::min<uint64_t>(1ull << 24, std::max<uint64_t>(1ull << 16, 4ull * max)));
    const uint32_t cap = (uint32_t)std::min<uint64_t>(max, R);
    auto grow = [](DevBuf &b, size_t want) -> int { return b.bytes >= want ? 0 : b.ensure(want); };
    int r;
    if ((r = grow(sel, R * 4)) || (r = grow(nsel, 8)) || (r = grow(dk, (size_t)cap * m.ksz)) || (r = grow(dv, (size_t)cap * m.vsz)))
        return r;
    gf_htab_desc d = m.hdesc();
    SlotFull pred{d.slots, start, d.slot_size, d.ksz};
    size_t tb = 0;
    (void)rocprim::select(nullptr, tb, rocprim::counting_iterator<uint32_t>(0u), (uint32_t *)sel.p, (uint32_t *)nsel.p,
                          (size_t)R, pred, (hipStream_t)0);
    if ((r = grow(tmp, tb + 256))) return r;
    tb = tmp.bytes;
    if (hip_ok(rocprim::select(tmp.p, tb, rocprim::counting_iterator<uint32_t>(0u), (uint32_t *)sel.p, (uint32_t *)nsel.p,
                               (size_t)R, pred, (hipStream_t)0), "dump select"))
        return -EIO;
    const uint32_t g2 = (uint32_t)std::min<uint64_t>((cap + BLOCK - 1) / BLOCK, 65535u);
    hipLaunchKernelGGL(k_dump_gather, dim3(g2 ? g2 : 1), dim3(BLOCK), 0, (hipStream_t)0, d, m.ht.codec, start,
                       (const uint32_t *)sel.p, (const uint32_t *)nsel.p, cap, (uint8_t *)dk.p, (uint8_t *)dv.p);
    if (hip_ok(hipGetLastError(), "k_dump_gather")) return -EIO;
    uint32_t ns = 0;
    if (hip_ok(hipMemcpy(&ns, nsel.p, 4, hipMemcpyDeviceToHost), "dump count")) return -EIO;
    const uint32_t got = std::min(ns, cap);
    m.xfer_d2h += 4 + (size_t)got * (m.ksz + m.vsz);
    if (got && (hip_ok(hipMemcpy(keys, dk.p, (size_t)got * m.ksz, hipMemcpyDeviceToHost), "dump keys") ||
                hip_ok(hipMemcpy(vals, dv.p, (size_t)got * m.vsz, hipMemcpyDeviceToHost), "dump vals")))
        return -EIO;
    if (ns > cap) {                                      // stopped inside the range: resume after the last one
        uint32_t last = 0;
        if (hip_ok(hipMemcpy(&last, (const uint32_t *)sel.p + (cap - 1), 4, hipMemcpyDeviceToHost), "dump last")) return -EIO;
        *next = start + last + 1;
    } else {
        *next = start + R;
    }
    *n = got;
    return 0;
}
}  // namespace gf
