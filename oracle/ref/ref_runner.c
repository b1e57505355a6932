/*
 * ref_runner.c — runs reference programs, compiled as host code into wrapper
 * objects (ref_bpf_*.c + ref_shim.h), over the frames and maps of a scenario,
 * one packet at a time in batch order as BPF would on one CPU, and writes what
 * each run left behind.  TEST INFRASTRUCTURE ONLY; our own code throughout.
 *
 *   ref_runner run  INPUT OUTPUT      (formats: oracle/refdiff.py input_bytes / read_output)
 *   ref_runner csum INPUT OUTPUT      (the three checksum helpers on given operands)
 *
 * Map semantics are the kernel's published ones (kernel/bpf/hashtab.c,
 * lpm_trie.c, arraymap.c): HASH / LRU_HASH exact match over key_size bytes,
 * LPM_TRIE longest prefix, flags BPF_ANY / BPF_NOEXIST / BPF_EXIST, a full HASH
 * is -E2BIG, a full trie -ENOSPC.  LRU eviction is NOT modelled: a scenario in
 * which an LRU map would reach its capacity is refused (exit status 3).
 * Checksums: RFC 1071 one's-complement sums, RFC 1624 incremental update.
 */
#define _GNU_SOURCE
#include <dlfcn.h>
#include <errno.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/mman.h>
#include "ref_rt.h"

#define MT_HASH 1
#define MT_ARRAY 2
#define MT_PROG_ARRAY 3
#define MT_LRU_HASH 9
#define MT_LPM_TRIE 11
#define F_ANY 0
#define F_NOEXIST 1
#define F_EXIST 2

static void die(const char *what)
{
    fprintf(stderr, "ref_runner: %s\n", what);
    exit(2);
}

/* ------------------------------------------------------------------ maps */
typedef struct hent { struct hent *next; uint8_t kv[]; } hent;
typedef struct hmap {
    char name[32];
    uint32_t type, ksz, vsz, voff, max_entries, count, nbuckets;   /* voff: the value's offset, 8-aligned as in the kernel */
    hent **bucket;
    uint8_t *array;             /* ARRAY / PROG_ARRAY values */
    hent *grave;                /* deleted while a program may still hold the value pointer */
} hmap;

static uint32_t hash_bytes(const uint8_t *p, uint32_t n)
{
    uint32_t h = 2166136261u;
    for (uint32_t i = 0; i < n; i++) h = (h ^ p[i]) * 16777619u;
    return h;
}

static hmap *hmap_new(const char *name, uint32_t type, uint32_t ksz, uint32_t vsz, uint32_t max_entries)
{
    hmap *m = calloc(1, sizeof *m);
    if (!m) die("out of memory");
    snprintf(m->name, sizeof m->name, "%s", name);
    m->type = type; m->ksz = ksz; m->vsz = vsz; m->voff = (ksz + 7) & ~7u; m->max_entries = max_entries;
    if (type == MT_ARRAY || type == MT_PROG_ARRAY) {
        if (ksz != 4) die("array map with a key that is not 4 bytes");
        m->array = calloc(max_entries ? max_entries : 1, vsz ? vsz : 1);
        if (!m->array) die("out of memory");
    } else if (type == MT_HASH || type == MT_LRU_HASH || type == MT_LPM_TRIE) {
        m->nbuckets = 4096;
        m->bucket = calloc(m->nbuckets, sizeof *m->bucket);
        if (!m->bucket) die("out of memory");
        if (type == MT_LPM_TRIE && ksz <= 4) die("LPM key without data");
    } else {
        die("unsupported map type");
    }
    return m;
}

/* an LPM key as the trie stores it: the bits past prefixlen do not take part */
static void lpm_norm(const hmap *m, const uint8_t *key, uint8_t *out)
{
    uint32_t plen, bits = (m->ksz - 4) * 8;
    memcpy(out, key, m->ksz);
    memcpy(&plen, key, 4);
    if (plen > bits) plen = bits;
    for (uint32_t b = 0; b < m->ksz - 4; b++) {
        int keep = (int)plen - (int)(8 * b);
        uint8_t mask = keep >= 8 ? 0xff : keep <= 0 ? 0 : (uint8_t)(0xff << (8 - keep));
        out[4 + b] &= mask;
    }
}

static hent **hmap_slot(hmap *m, const uint8_t *key)
{
    hent **pp = &m->bucket[hash_bytes(key, m->ksz) % m->nbuckets];
    while (*pp && memcmp((*pp)->kv, key, m->ksz)) pp = &(*pp)->next;
    return pp;
}

static void *hmap_lookup(hmap *m, const void *key_)
{
    const uint8_t *key = key_;
    if (m->type == MT_ARRAY) {
        uint32_t i; memcpy(&i, key, 4);
        return i < m->max_entries ? m->array + (size_t)i * m->vsz : NULL;
    }
    if (m->type == MT_PROG_ARRAY) return NULL;       /* programs cannot read a prog array */
    if (m->type == MT_LPM_TRIE) {
        uint8_t k[64];
        uint32_t plen, bits = (m->ksz - 4) * 8;
        memcpy(&plen, key, 4);
        if (plen > bits) plen = bits;
        for (int p = (int)plen; p >= 0; p--) {      /* longest stored prefix that covers the key */
            uint32_t pl = (uint32_t)p;
            memcpy(k, key, m->ksz);
            memcpy(k, &pl, 4);
            lpm_norm(m, k, k);
            hent *e = *hmap_slot(m, k);
            if (e) return e->kv + m->voff;
        }
        return NULL;
    }
    hent *e = *hmap_slot(m, key);
    return e ? e->kv + m->voff : NULL;
}

static int hmap_update(hmap *m, const void *key_, const void *value, uint64_t flags)
{
    const uint8_t *key = key_;
    uint8_t k[64];
    if (flags > F_EXIST) return -EINVAL;
    if (m->type == MT_ARRAY) {
        uint32_t i; memcpy(&i, key, 4);
        if (i >= m->max_entries) return -E2BIG;
        if (flags == F_NOEXIST) return -EEXIST;
        memcpy(m->array + (size_t)i * m->vsz, value, m->vsz);
        return 0;
    }
    if (m->type == MT_PROG_ARRAY) return -EINVAL;
    if (m->type == MT_LPM_TRIE) {
        uint32_t plen; memcpy(&plen, key, 4);
        if (plen > (m->ksz - 4) * 8) return -EINVAL;
        lpm_norm(m, key, k);
        key = k;
    }
    hent **pp = hmap_slot(m, key);
    if (*pp) {
        if (flags == F_NOEXIST) return -EEXIST;
        memcpy((*pp)->kv + m->voff, value, m->vsz);
        return 0;
    }
    if (flags == F_EXIST) return -ENOENT;
    if (m->count >= m->max_entries) {
        if (m->type == MT_LRU_HASH) {
            fprintf(stderr, "ref_runner: LRU map %s reached its capacity: eviction is not modelled\n", m->name);
            exit(3);
        }
        return m->type == MT_LPM_TRIE ? -ENOSPC : -E2BIG;
    }
    hent *e = malloc(sizeof *e + m->voff + m->vsz);
    if (!e) die("out of memory");
    e->next = NULL;
    memcpy(e->kv, key, m->ksz);
    memcpy(e->kv + m->voff, value, m->vsz);
    *pp = e;
    m->count++;
    return 0;
}

static int hmap_delete(hmap *m, const void *key_)
{
    const uint8_t *key = key_;
    uint8_t k[64];
    if (m->type == MT_ARRAY || m->type == MT_PROG_ARRAY) return -EINVAL;
    if (m->type == MT_LPM_TRIE) { lpm_norm(m, key, k); key = k; }
    hent **pp = hmap_slot(m, key);
    if (!*pp) return -ENOENT;
    hent *e = *pp;
    *pp = e->next;
    e->next = m->grave;         /* the kernel frees after an RCU grace period */
    m->grave = e;
    m->count--;
    return 0;
}

static void hmap_reap(hmap *m)
{
    while (m->grave) { hent *e = m->grave; m->grave = e->next; free(e); }
}

static void hmap_free(hmap *m)
{
    hmap_reap(m);
    for (uint32_t b = 0; b < m->nbuckets; b++)
        while (m->bucket[b]) { hent *e = m->bucket[b]; m->bucket[b] = e->next; free(e); }
    free(m->bucket); free(m->array); free(m);
}

/* ------------------------------------------------------------------ checksums */
/* RFC 1071: the sum is taken over 16-bit words in memory order with end-around carry. */
static uint32_t add32(uint32_t a, uint32_t b)
{
    uint64_t s = (uint64_t)a + b;
    return (uint32_t)(s & 0xffffffffu) + (uint32_t)(s >> 32);
}
static uint16_t fold16(uint32_t s)
{
    s = (s & 0xffff) + (s >> 16);
    s = (s & 0xffff) + (s >> 16);
    return (uint16_t)s;
}
static uint32_t sum_words(const uint8_t *p, uint32_t n, uint32_t seed, int complement)
{
    uint32_t s = seed;
    for (uint32_t i = 0; i + 4 <= n; i += 4) {
        uint32_t w; memcpy(&w, p + i, 4);
        s = add32(s, complement ? ~w : w);
    }
    return s;
}

/* bpf_csum_diff: seed + sum(to) - sum(from) as a 32-bit one's-complement sum; sizes are multiples of 4 */
static int rt_csum_diff(const void *from, uint32_t from_size, const void *to, uint32_t to_size, uint32_t seed)
{
    if (((from_size | to_size) & 3) || from_size + to_size > 512) return -EINVAL;
    uint32_t s = sum_words(from, from_size, seed, 1);
    return (int)sum_words(to, to_size, s, 0);
}

/* RFC 1624 eqn. 3: HC' = ~(~HC + ~m + m') */
static uint16_t csum_update(uint16_t hc, uint32_t from, uint32_t to)
{
    uint32_t s = add32(add32((uint16_t)~hc, ~from), to);
    return (uint16_t)~fold16(s);
}

#define CS_HDR_FIELD_MASK 0xfull
#define CS_PSEUDO_HDR (1ull << 4)
#define CS_MARK_MANGLED_0 (1ull << 5)
#define CS_MARK_ENFORCE (1ull << 6)

static int rt_l3_csum_replace(uint8_t *pkt, uint32_t len, uint32_t off, uint32_t from, uint32_t to, uint64_t flags)
{
    uint16_t hc;
    if (flags & ~CS_HDR_FIELD_MASK) return -EINVAL;
    if (off > 0xffff || (off & 1)) return -EFAULT;
    if ((uint64_t)off + 2 > len) return -EFAULT;
    memcpy(&hc, pkt + off, 2);
    switch (flags & CS_HDR_FIELD_MASK) {
    case 0: if (from) return -EINVAL; hc = csum_update(hc, 0, to); break;
    case 2: hc = csum_update(hc, from & 0xffff, to & 0xffff); break;
    case 4: hc = csum_update(hc, from, to); break;
    default: return -EINVAL;
    }
    memcpy(pkt + off, &hc, 2);
    return 0;
}

static int rt_l4_csum_replace(uint8_t *pkt, uint32_t len, uint32_t off, uint32_t from, uint32_t to, uint64_t flags)
{
    uint16_t hc;
    int mm0 = (flags & CS_MARK_MANGLED_0) != 0, force = (flags & CS_MARK_ENFORCE) != 0;
    if (flags & ~(CS_MARK_MANGLED_0 | CS_MARK_ENFORCE | CS_PSEUDO_HDR | CS_HDR_FIELD_MASK)) return -EINVAL;
    if (off > 0xffff || (off & 1)) return -EFAULT;
    if ((uint64_t)off + 2 > len) return -EFAULT;
    memcpy(&hc, pkt + off, 2);
    if (mm0 && !force && !hc) return 0;             /* a UDP checksum of 0 means "none": left alone */
    switch (flags & CS_HDR_FIELD_MASK) {
    case 0: if (from) return -EINVAL; hc = csum_update(hc, 0, to); break;
    case 2: hc = csum_update(hc, from & 0xffff, to & 0xffff); break;
    case 4: hc = csum_update(hc, from, to); break;
    default: return -EINVAL;
    }
    if (mm0 && !hc) hc = 0xffff;                    /* CSUM_MANGLED_0 */
    memcpy(pkt + off, &hc, 2);
    return 0;
}

/* ------------------------------------------------------------------ runtime */
#define MAX_MAPS 256
#define MAX_BINDS 1024
typedef struct runner {
    struct ref_rt rt;           /* first: the callbacks get it back */
    hmap *maps[MAX_MAPS]; uint32_t nmaps;
    struct { const void *obj; hmap *m; } binds[MAX_BINDS]; uint32_t nbinds;
    uint64_t now_ns;
    uint64_t rng;
    uint8_t *ev; size_t ev_len, ev_cap;
} runner;

static hmap *find_map(runner *r, const char *name)
{
    for (uint32_t i = 0; i < r->nmaps; i++)
        if (!strcmp(r->maps[i]->name, name)) return r->maps[i];
    return NULL;
}

static hmap *bound(runner *r, const void *obj)
{
    for (uint32_t i = 0; i < r->nbinds; i++)
        if (r->binds[i].obj == obj) return r->binds[i].m;
    return NULL;
}

static uint32_t cb_bind(struct ref_rt *rt, const void *obj, const char *name)
{
    runner *r = (runner *)rt;
    if (r->nbinds >= MAX_BINDS) die("too many bound maps");
    r->binds[r->nbinds].obj = obj;
    r->binds[r->nbinds].m = find_map(r, name);       /* NULL: reaching it is "unmodelled" */
    return r->nbinds++;
}

static uint32_t cb_bind_index(struct ref_rt *rt, const void *obj)
{
    runner *r = (runner *)rt;
    for (uint32_t i = 0; i < r->nbinds; i++)
        if (r->binds[i].obj == obj) return i;
    return ~0u;
}

static void *cb_lookup(struct ref_rt *rt, const void *obj, const void *key)
{
    hmap *m = bound((runner *)rt, obj);
    if (!m) { rt->cur.unmodelled = 1; return NULL; }
    return hmap_lookup(m, key);
}
static int cb_update(struct ref_rt *rt, const void *obj, const void *key, const void *value, uint64_t flags)
{
    hmap *m = bound((runner *)rt, obj);
    if (!m) { rt->cur.unmodelled = 1; return -EINVAL; }
    return hmap_update(m, key, value, flags);
}
static int cb_delete(struct ref_rt *rt, const void *obj, const void *key)
{
    hmap *m = bound((runner *)rt, obj);
    if (!m) { rt->cur.unmodelled = 1; return -EINVAL; }
    return hmap_delete(m, key);
}
static uint64_t cb_ktime(struct ref_rt *rt) { return ((runner *)rt)->now_ns; }
static uint32_t cb_prandom(struct ref_rt *rt)
{
    runner *r = (runner *)rt;                        /* splitmix64, seeded per run */
    uint64_t z = (r->rng += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return (uint32_t)((z ^ (z >> 31)) >> 32);
}
static void ev_put(runner *r, const void *p, size_t n)
{
    if (r->ev_len + n > r->ev_cap) {
        r->ev_cap = (r->ev_len + n) * 2 + 4096;
        r->ev = realloc(r->ev, r->ev_cap);
        if (!r->ev) die("out of memory");
    }
    memcpy(r->ev + r->ev_len, p, n);
    r->ev_len += n;
}
/* one event: u32 meta_size, u32 cap, the metadata, the captured packet bytes */
static void cb_event(struct ref_rt *rt, const void *meta, uint32_t meta_size, const uint8_t *pkt, uint32_t cap)
{
    runner *r = (runner *)rt;
    ev_put(r, &meta_size, 4); ev_put(r, &cap, 4);
    ev_put(r, meta, meta_size); ev_put(r, pkt, cap);
}

/* ------------------------------------------------------------------ I/O */
static void rd(FILE *f, void *p, size_t n) { if (n && fread(p, 1, n, f) != n) die("short input"); }
static uint32_t rd32(FILE *f) { uint32_t v; rd(f, &v, 4); return v; }
static uint64_t rd64(FILE *f) { uint64_t v; rd(f, &v, 8); return v; }
static void wr(FILE *f, const void *p, size_t n) { if (n && fwrite(p, 1, n, f) != n) die("short write"); }
static void wr32(FILE *f, uint32_t v) { wr(f, &v, 4); }

static uint32_t g_ksz;
static int cmp_rows(const void *a, const void *b) { return memcmp(*(uint8_t *const *)a, *(uint8_t *const *)b, g_ksz); }

static void dump_map(FILE *f, hmap *m)
{
    char name[32] = {0};
    snprintf(name, sizeof name, "%s", m->name);
    wr(f, name, 32); wr32(f, m->ksz); wr32(f, m->vsz);
    if (m->type == MT_ARRAY || m->type == MT_PROG_ARRAY) {
        wr32(f, m->max_entries);
        for (uint32_t i = 0; i < m->max_entries; i++) wr32(f, i);
        wr(f, m->array, (size_t)m->max_entries * m->vsz);
        return;
    }
    uint8_t **rows = malloc(sizeof *rows * (m->count ? m->count : 1));
    if (!rows) die("out of memory");
    uint32_t n = 0;
    for (uint32_t b = 0; b < m->nbuckets; b++)
        for (hent *e = m->bucket[b]; e; e = e->next) rows[n++] = e->kv;
    g_ksz = m->ksz;
    qsort(rows, n, sizeof *rows, cmp_rows);
    wr32(f, n);
    for (uint32_t i = 0; i < n; i++) wr(f, rows[i], m->ksz);
    for (uint32_t i = 0; i < n; i++) wr(f, rows[i] + m->voff, m->vsz);
    free(rows);
}

#define PKT_AREA (1u << 16)

typedef struct prog { void *dl; ref_run_fn run; uint32_t slot; } prog;

static int run_mode(const char *in_path, const char *out_path)
{
    FILE *in = fopen(in_path, "rb"), *out = fopen(out_path, "wb");
    if (!in || !out) die("cannot open input / output");
    runner *r = calloc(1, sizeof *r);
    if (!r) die("out of memory");
    r->rt.map_lookup = cb_lookup; r->rt.map_update = cb_update; r->rt.map_delete = cb_delete;
    r->rt.bind = cb_bind; r->rt.bind_index = cb_bind_index; r->rt.ktime_get_ns = cb_ktime;
    r->rt.prandom = cb_prandom; r->rt.event = cb_event; r->rt.csum_diff = rt_csum_diff;
    r->rt.l3_csum_replace = rt_l3_csum_replace; r->rt.l4_csum_replace = rt_l4_csum_replace;

    if (rd32(in) != 0x49524647u) die("bad magic");   /* "GFRI" */
    r->rng = rd64(in);
    uint32_t route = rd32(in);                        /* 1: by the packet's lxc_id column, 0: the first program */
    r->nmaps = rd32(in);
    if (r->nmaps > MAX_MAPS) die("too many maps");
    for (uint32_t i = 0; i < r->nmaps; i++) {
        char name[33] = {0};
        rd(in, name, 32);
        uint32_t type = rd32(in), ksz = rd32(in), vsz = rd32(in), max_entries = rd32(in), n = rd32(in);
        if (ksz > 64 || vsz > 4096) die("map key / value too large");
        hmap *m = r->maps[i] = hmap_new(name, type, ksz, vsz, max_entries);
        uint8_t *k = malloc((size_t)n * ksz + 1), *v = malloc((size_t)n * vsz + 1);
        if (!k || !v) die("out of memory");
        rd(in, k, (size_t)n * ksz); rd(in, v, (size_t)n * vsz);
        for (uint32_t j = 0; j < n; j++)
            if (hmap_update(m, k + (size_t)j * ksz, v + (size_t)j * vsz, F_ANY) < 0) die("map load failed");
        free(k); free(v);
    }
    uint32_t nprogs = rd32(in);
    prog *progs = calloc(nprogs ? nprogs : 1, sizeof *progs);
    if (!progs) die("out of memory");
    for (uint32_t i = 0; i < nprogs; i++) {
        char path[513] = {0};
        progs[i].slot = rd32(in);
        rd(in, path, 512);
        progs[i].dl = dlopen(path, RTLD_NOW | RTLD_LOCAL);
        if (!progs[i].dl) { fprintf(stderr, "%s\n", dlerror()); die("cannot load a program object"); }
        ref_bind_fn bind = (ref_bind_fn)dlsym(progs[i].dl, "ref_bind");
        progs[i].run = (ref_run_fn)dlsym(progs[i].dl, "ref_run");
        if (!bind || !progs[i].run) die("program object without ref_bind / ref_run");
        bind(&r->rt);
    }
    /* map names in bind order, so that a recorded tail call can be named */
    wr32(out, 0x4f524647u);                           /* "GFRO" */
    wr32(out, r->nbinds);
    for (uint32_t i = 0; i < r->nbinds; i++) {
        char name[32] = {0};
        if (r->binds[i].m) snprintf(name, sizeof name, "%s", r->binds[i].m->name);
        wr(out, name, 32);
    }

    /* packet memory below 4 GiB, a guard page behind it: the frame ends where the guard begins */
    uint8_t *area = mmap(NULL, PKT_AREA + 4096, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_32BIT, -1, 0);
    if (area == MAP_FAILED || (uintptr_t)area + PKT_AREA + 4096 > 0xffffffffull) die("no packet memory below 4 GiB");
    if (mprotect(area + PKT_AREA, 4096, PROT_NONE)) die("mprotect");

    uint32_t nbatches = rd32(in);
    wr32(out, nbatches);
    for (uint32_t bi = 0; bi < nbatches; bi++) {
        uint32_t n = rd32(in), stride = rd32(in);
        r->now_ns = rd64(in);
        size_t fb = (size_t)n * stride;
        uint8_t *frames = malloc(fb + 1);
        uint32_t *col = malloc(((size_t)n * 7 + 1) * 4);
        struct ref_obs *obs = calloc(n ? n : 1, sizeof *obs);
        uint32_t *ev_off = calloc((size_t)n + 1, 4);
        if (!frames || !col || !obs || !ev_off) die("out of memory");
        rd(in, frames, fb);
        rd(in, col, (size_t)n * 7 * 4);
        const uint32_t *len = col, *sid = col + n, *ifx = col + 2 * (size_t)n, *lxc = col + 3 * (size_t)n,
                       *tci = col + 4 * (size_t)n, *fh = col + 5 * (size_t)n, *mark = col + 6 * (size_t)n;
        r->ev_len = 0;
        for (uint32_t i = 0; i < n; i++) {
            prog *p = NULL;
            if (!route) p = nprogs ? &progs[0] : NULL;
            else for (uint32_t k = 0; k < nprogs; k++) if (progs[k].slot == lxc[i]) { p = &progs[k]; break; }
            ev_off[i] = (uint32_t)r->ev_len;
            memset(&r->rt.cur, 0, sizeof r->rt.cur);
            if (!p) { obs[i].ret = INT32_MIN + 1; continue; }   /* no program in that slot: not run */
            if (len[i] > PKT_AREA) die("frame longer than the packet area");
            uint32_t have = len[i] < stride ? len[i] : stride;
            uint8_t *data = area + PKT_AREA - len[i];
            memset(data, 0, len[i]);
            memcpy(data, frames + (size_t)i * stride, have);
            struct ref_pkt pk;
            memset(&pk, 0, sizeof pk);
            pk.data = data; pk.len = len[i];
            if (len[i] >= 14) pk.protocol = (uint32_t)data[12] | ((uint32_t)data[13] << 8);
            pk.cb[0] = sid[i]; pk.cb[1] = ifx[i];
            pk.tc_index = tci[i]; pk.hash = fh[i]; pk.mark = mark[i];
            p->run(&r->rt, &pk);
            obs[i] = r->rt.cur;
            memcpy(frames + (size_t)i * stride, data, have);
            for (uint32_t k = 0; k < r->nmaps; k++) hmap_reap(r->maps[k]);
        }
        ev_off[n] = (uint32_t)r->ev_len;
        wr32(out, n); wr32(out, stride);
        wr(out, obs, (size_t)n * sizeof *obs);
        wr(out, frames, fb);
        wr(out, ev_off, ((size_t)n + 1) * 4);
        wr(out, r->ev, r->ev_len);
        wr32(out, r->nmaps);
        for (uint32_t k = 0; k < r->nmaps; k++) dump_map(out, r->maps[k]);
        free(frames); free(col); free(obs); free(ev_off);
    }
    munmap(area, PKT_AREA + 4096);
    for (uint32_t i = 0; i < nprogs; i++) dlclose(progs[i].dl);
    for (uint32_t k = 0; k < r->nmaps; k++) hmap_free(r->maps[k]);
    free(progs); free(r->ev); free(r);
    fclose(in);
    if (fclose(out)) die("close failed");
    return 0;
}

/* csum mode.  Input: u32 n, then n records of
 *   u32 op (0 csum_diff, 1 l3, 2 l4), u32 a, u32 b, u32 c, u32 d, u8 buf[64]
 * op 0: a = from_size, b = to_size, c = seed; from at buf, to at buf + 32
 * op 1/2: a = off, b = from, c = to, d = flags; the packet is buf, 64 bytes long
 * Output per record: i32 ret, u8 buf[64] as left. */
static int csum_mode(const char *in_path, const char *out_path)
{
    FILE *in = fopen(in_path, "rb"), *out = fopen(out_path, "wb");
    if (!in || !out) die("cannot open input / output");
    uint32_t n = rd32(in);
    for (uint32_t i = 0; i < n; i++) {
        uint32_t op = rd32(in), a = rd32(in), b = rd32(in), c = rd32(in), d = rd32(in);
        uint8_t buf[64];
        int32_t ret;
        rd(in, buf, 64);
        if (op == 0) ret = (a > 32 || b > 32) ? -EINVAL : rt_csum_diff(buf, a, buf + 32, b, c);
        else if (op == 1) ret = rt_l3_csum_replace(buf, 64, a, b, c, d);
        else ret = rt_l4_csum_replace(buf, 64, a, b, c, d);
        wr(out, &ret, 4); wr(out, buf, 64);
    }
    fclose(in);
    if (fclose(out)) die("close failed");
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 4 && !strcmp(argv[1], "run")) return run_mode(argv[2], argv[3]);
    if (argc == 4 && !strcmp(argv[1], "csum")) return csum_mode(argv[2], argv[3]);
    fprintf(stderr, "usage: ref_runner run|csum INPUT OUTPUT\n");
    return 64;
}
