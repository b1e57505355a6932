/*
 * ref_rt.h — the interface between the helper shim (ref_shim.h, compiled into
 * each wrapper translation unit next to one reference program) and the runner
 * (ref_runner.c), which owns the host maps, the packet memory, the event log
 * and the checksum arithmetic.  TEST INFRASTRUCTURE ONLY.
 *
 * Nothing here comes from the reference tree: the wrapper units reach it only
 * through #include names resolved by -I at build time (oracle/refdiff.py).
 */
#ifndef GF_REF_RT_H
#define GF_REF_RT_H
#include <stdint.h>

#define REF_NCB 5

/* what one program run leaves behind besides the frame and the maps */
struct ref_obs {
    int32_t  ret;
    uint32_t redirect_called, redirect_ifindex, redirect_flags;
    uint32_t tail_called, tail_map, tail_index;     /* tail_map: bind index of the map, ~0u unknown */
    uint32_t cb[REF_NCB];
    uint32_t unmodelled;                            /* an unmodelled helper / unbound map was reached */
};

/* one packet as the runner hands it to a program */
struct ref_pkt {
    uint8_t *data;              /* below 4 GiB: __sk_buff.data / xdp_md.data are 32 bit */
    uint32_t len;
    uint32_t protocol;          /* __sk_buff.protocol (network order in the low 16 bits) */
    uint32_t cb[REF_NCB];
    uint32_t tc_index, hash, ifindex, ingress_ifindex, mark;
};

struct ref_rt {
    /* maps: `map` is the address of the program's own map object */
    void *(*map_lookup)(struct ref_rt *, const void *map, const void *key);
    int   (*map_update)(struct ref_rt *, const void *map, const void *key, const void *value, uint64_t flags);
    int   (*map_delete)(struct ref_rt *, const void *map, const void *key);
    /* registration, called by the unit's ref_bind(): map object -> scenario map name; returns the bind index */
    uint32_t (*bind)(struct ref_rt *, const void *map, const char *name);
    uint32_t (*bind_index)(struct ref_rt *, const void *map);
    uint64_t (*ktime_get_ns)(struct ref_rt *);
    uint32_t (*prandom)(struct ref_rt *);
    void  (*event)(struct ref_rt *, const void *meta, uint32_t meta_size, const uint8_t *pkt, uint32_t cap);
    /* checksum arithmetic on plain buffers (RFC 1071 / RFC 1624) */
    int   (*csum_diff)(const void *from, uint32_t from_size, const void *to, uint32_t to_size, uint32_t seed);
    int   (*l3_csum_replace)(uint8_t *pkt, uint32_t len, uint32_t off, uint32_t from, uint32_t to, uint64_t flags);
    int   (*l4_csum_replace)(uint8_t *pkt, uint32_t len, uint32_t off, uint32_t from, uint32_t to, uint64_t flags);
    struct ref_obs cur;         /* the packet being run */
};

/* what every wrapper unit exports */
typedef void (*ref_bind_fn)(struct ref_rt *);
typedef void (*ref_run_fn)(struct ref_rt *, struct ref_pkt *);
#define REF_KIND_SKB 0
#define REF_KIND_XDP 1

#endif
