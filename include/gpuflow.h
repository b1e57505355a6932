/*
 * gpuflow.h — C ABI of libgpuflow, the MI355X-native replacement for the
 * kernel side of Cilium's BPF map syscalls and its per-packet verdict
 * programs (reference: carlanton/cilium 1.0.0-rc9, /root/reference).
 *
 * Plain C: pointers, sizes and integer handles only.  Every entry point
 * returns 0 / a positive handle on success and -errno on failure, the way
 * the bpf(2) syscall wrappers in pkg/bpf/bpf.go see the kernel.
 *
 * Two groups of entry points:
 *
 *  1. Map API (drop-in for pkg/bpf/bpf.go) — host shadow + HBM replica.
 *     gf_map_create        <- bpf.CreateMap        pkg/bpf/bpf.go:84-112
 *     gf_map_update_elem   <- bpf.UpdateElement    pkg/bpf/bpf.go:129-149
 *     gf_map_lookup_elem   <- bpf.LookupElement    pkg/bpf/bpf.go:153-172
 *     gf_map_delete_elem   <- bpf.DeleteElement    pkg/bpf/bpf.go:175-192
 *     gf_map_get_next_key  <- bpf.GetNextKey       pkg/bpf/bpf.go:195-213
 *     gf_obj_pin           <- bpf.ObjPin           pkg/bpf/bpf.go:224-243
 *     gf_obj_get           <- bpf.ObjGet           pkg/bpf/bpf.go:246-266
 *     gf_obj_close         <- bpf.ObjClose         pkg/bpf/bpf.go:269-274
 *     gf_map_get_info      <- bpf.GetMapInfo       pkg/bpf/map.go:171-209 (fdinfo parse)
 *     gf_map_lookup_batch  <- the GetNextKey + LookupElement loop of bpf.Map.DumpWithCallback
 *                             pkg/bpf/map.go:319-369, in chunks
 *     gf_now_sec           <- bpf.GetMtime()/1e9   pkg/bpf/bpf.go:426-435, bpf/lib/utils.h:58-64
 *
 *  2. Program API (replaces the BPF programs of the hot path).  A "program"
 *     binds map handles the way the compile-time #defines of the generated
 *     headers do (pkg/endpoint/bpf.go:156-330, bpf/filter_config.h,
 *     bpf/lxc_config.h, bpf/netdev_config.h); a classify call runs the
 *     program over one batch of packets that is resident in HBM.
 *     gf_xdp_classify            <- xdp_start/check_filters   bpf/bpf_xdp.c:88-184
 *     gf_xdp_filter_frames       <- the same over raw frames: the XDP_PASS frames packed in arrival order
 *     gf_lb_classify             <- from_netdev (bpf_lb)      bpf/bpf_lb.c:58-212
 *     gf_lb_classify_frames      <- the same over raw frames, with lb*_xlate's rewrites and LB_DSTMAC
 *     gf_policy_ingress_classify <- handle_policy/ipv{4,6}_policy bpf/bpf_lxc.c:745-1024
 *     gf_lxc_egress_classify     <- from-container handle_ingress bpf/bpf_lxc.c:427-738
 *     gf_pipeline_classify       <- bpf_xdp -> bpf_lb -> bpf_netdev -> cilium_policy tail call
 *     gf_overlay_classify        <- from_overlay (tunnel receive) bpf/bpf_overlay.c:38-200 -> cilium_policy
 *                                   tail call (VXLAN; no DROP_NO_TUNNEL_KEY, no Geneve options)
 *     gf_host_classify           <- from_netdev with FROM_HOST (cilium_host) bpf/bpf_netdev.c:50-468 ->
 *                                   cilium_policy tail call (the proxy return path; no HANDLE_NS)
 *     gf_parse_frames            <- the skb_load_bytes()/revalidate_data() header
 *                                   accesses of those programs (bpf/lib/common.h:67-87,
 *                                   bpf/lib/ipv4.h:45-48, bpf/lib/ipv6.h:61-98)
 *     gf_forward_queues / gf_forward_frames <- what the verdict does to the skb: SHOT frees it, OK hands
 *                                   it to the stack, redirect(ifindex) queues it on that device
 *
 * Host/device contract: map updates go to the host shadow and are pushed to
 * the HBM replica at the next classify call (batch boundary; a documented
 * relaxation of the kernel's per-element RCU visibility).  Maps the
 * datapath writes (CT entries, policy counters) are device-authoritative:
 * host-side lookups, updates, deletes and get_next_key then walk the key's
 * probe sequence in HBM with small reads / writes, and dumps stream in chunks
 * selected on the device; no call copies a whole table.  Each map has its own
 * lock; a classify call holds the locks of the maps its programs bind.
 *
 * All batch/column/output pointers passed to classify calls are DEVICE
 * pointers (hipMalloc / torch CUDA tensors).  `stream` is a hipStream_t
 * (NULL = default stream).  Classify calls are asynchronous w.r.t. the host
 * except for the table sync they may perform before launching.
 */
#ifndef GPUFLOW_H
#define GPUFLOW_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- map types (enum bpf_map_type subset, pkg/bpf/bpf.go:38-52) ---- */
#define GF_MAP_TYPE_HASH      1
#define GF_MAP_TYPE_ARRAY     2
#define GF_MAP_TYPE_PROG_ARRAY 3
#define GF_MAP_TYPE_LRU_HASH  9
#define GF_MAP_TYPE_LPM_TRIE  11

/* update flags (pkg/bpf/bpf.go:73-75) */
#define GF_ANY     0
#define GF_NOEXIST 1
#define GF_EXIST   2

/* map flags (pkg/bpf/bpf.go:77-78) */
#define GF_F_NO_PREALLOC   (1u << 0)
#define GF_F_NO_COMMON_LRU (1u << 1)

/* ---- return codes of the datapath (bpf/include/bpf/api.h:17-25,
 *      bpf/include/linux/bpf.h:622-624) ---- */
#define GF_TC_ACT_OK        0
#define GF_TC_ACT_SHOT      2
#define GF_TC_ACT_REDIRECT  7
#define GF_XDP_DROP         1
#define GF_XDP_PASS         2

/* CT lookup results (bpf/lib/common.h:310-315) */
#define GF_CT_NEW         0
#define GF_CT_ESTABLISHED 1
#define GF_CT_REPLY       2
#define GF_CT_RELATED     3

/* drop reasons are reported as u8 = -DROP_* (bpf/lib/common.h:224-256) */
#define GF_DROP_INVALID            134
#define GF_DROP_POLICY             133
#define GF_DROP_CT_INVALID_HDR     135
#define GF_DROP_CT_UNKNOWN_PROTO   137
#define GF_DROP_UNKNOWN_L3         139
#define GF_DROP_MISSED_TAIL_CALL   140
#define GF_DROP_WRITE_ERROR        141
#define GF_DROP_UNKNOWN_L4         142
#define GF_DROP_CSUM_L3            153
#define GF_DROP_CSUM_L4            154
#define GF_DROP_CT_CREATE_FAILED   155
#define GF_DROP_INVALID_EXTHDR     156
#define GF_DROP_FRAG_NOSUPPORT     157
#define GF_DROP_NO_SERVICE         158
#define GF_DROP_POLICY_L4          159

/* ======================= 1. Map API ======================= */

/* bpf.CreateMap: returns handle > 0 or -errno.  key/value sizes are the
 * byte sizes of the reference C structs (bpf/lib/common.h). */
int gf_map_create(uint32_t map_type, uint32_t key_size, uint32_t value_size,
                  uint32_t max_entries, uint32_t map_flags);
/* bpf.UpdateElement: flags GF_ANY/GF_NOEXIST/GF_EXIST.  -E2BIG when a
 * hash map is full, -ENOSPC for a full LPM trie, -EEXIST/-ENOENT under
 * NOEXIST/EXIST, -EINVAL for bad flags or an LPM prefixlen > max. */
int gf_map_update_elem(int map, const void *key, const void *value, uint64_t flags);
/* bpf.LookupElement: copies the value; -ENOENT if absent.  LPM tries use
 * longest-prefix semantics on key->prefixlen (kernel trie_lookup_elem). */
int gf_map_lookup_elem(int map, const void *key, void *value);
/* bpf.DeleteElement: -ENOENT if absent. */
int gf_map_delete_elem(int map, const void *key);
/* bpf.GetNextKey: key == NULL or an absent key -> first key; -ENOENT at end. */
int gf_map_get_next_key(int map, const void *key, void *next_key);
/* Batched update (same semantics as n sequential gf_map_update_elem calls;
 * stops at the first error and returns it, *n_done = entries applied). */
int gf_map_update_batch(int map, const void *keys, const void *values,
                        uint32_t n, uint64_t flags, uint32_t *n_done);

/* Chunked dump (what bpf.Map.DumpWithCallback, pkg/bpf/map.go:319-369, gets
 * from one GetNextKey + LookupElement pair per entry; the kernel's later
 * BPF_MAP_LOOKUP_BATCH contract): copies up to *count entries after the
 * opaque cursor *in_batch (NULL = from the start) into keys / values (host
 * arrays, reference layouts), sets *count to the number copied and *out_batch
 * to the cursor to resume from.  Returns 0, or -ENOENT once the map holds no
 * entry past the cursor (*count may still be > 0).  Device-authoritative maps
 * are compacted on the device; only the entries cross PCIe. */
int gf_map_lookup_batch(int map, const uint64_t *in_batch, uint64_t *out_batch,
                        void *keys, void *values, uint32_t *count);

typedef struct gf_map_info {
    uint32_t map_type, key_size, value_size, max_entries, map_flags;
    uint32_t n_entries;        /* current element count */
    uint64_t device_bytes;     /* HBM bytes of the replica (0 if never synced) */
    uint64_t xfer_d2h;         /* bytes the map API has copied device -> host (element walks, */
    uint64_t xfer_h2d;         /* dumps, pulls) and host -> device (element writes, pushes) */
} gf_map_info;
int gf_map_get_info(int map, gf_map_info *info);

/* bpf.ObjPin / ObjGet / ObjClose.  Pin paths are names in a process-wide
 * registry that stands in for /sys/fs/bpf (pkg/bpf/bpffs.go:35-38). */
int gf_obj_pin(int handle, const char *path);
int gf_obj_get(const char *path);          /* new handle referring to the object */
int gf_obj_close(int handle);
int gf_obj_unpin(const char *path);        /* os.Remove(path) of a pinned map */

/* CLOCK_MONOTONIC seconds, the clock bpf_ktime_get_sec() reads. */
uint32_t gf_now_sec(void);

/* ======================= 2. Programs ======================= */

/* Parsed header columns.  One element per packet; all DEVICE pointers.
 * Produced from raw frames by gf_parse_frames (or by a NIC/ingest stage
 * with the same rules).  "be16"/"be32" fields hold the raw network-order
 * bytes of the frame loaded little-endian, exactly what the BPF programs
 * hold in their registers after skb_load_bytes(). */
typedef struct gf_pkt_cols {
    uint32_t n;
    const uint32_t *len;        /* skb->len (linear == data_end - data) */
    const uint16_t *ethertype;  /* host order: 0x0800 / 0x86DD / other; 0 if len < 14 */
    const uint32_t *saddr4;     /* iphdr.saddr (raw be32), v4 only */
    const uint32_t *daddr4;     /* iphdr.daddr (raw be32), v4 only */
    const uint8_t  *proto;      /* v4: protocol; v6: nexthdr after ipv6_hdrlen() (unchanged on error) */
    const int16_t  *l4_off;     /* v4: 14 + ihl*4; v6: 14 + ipv6_hdrlen() (negative DROP_* on error) */
    const uint32_t *l4w0;       /* frame bytes [l4_off, l4_off+4) (0-filled past len) */
    const uint16_t *l4w3;       /* frame bytes [l4_off+12, l4_off+14) (TCP flags word) */
    const uint8_t  *saddr6;     /* 16 B per packet, v6 (may be NULL if no IPv6 in batch) */
    const uint8_t  *daddr6;     /* 16 B per packet, v6 */
    /* skb metadata the calling programs provide */
    const uint32_t *src_identity; /* cb[CB_SRC_LABEL] (bpf/lib/l3.h:160) */
    const uint32_t *ifindex;      /* cb[CB_IFINDEX]  (bpf/lib/l3.h:161) */
    const uint16_t *lxc_id;       /* tail-call slot into cilium_policy (bpf/lib/l3.h:163) */
    const uint8_t  *tc_index;     /* skb->tc_index (TC_INDEX_F_SKIP_PROXY = bit 0) */
    const uint32_t *flow_hash;    /* get_hash_recalc(skb) (bpf/lib/lb.h:109-121) */
} gf_pkt_cols;

/* Raw frames: snap_stride bytes per packet starting at the Ethernet header. */
typedef struct gf_frames {
    uint32_t n;
    uint32_t snap_stride;       /* >= all header bytes the programs read */
    const uint8_t  *snap;       /* n * snap_stride bytes */
    const uint32_t *len;        /* wire length of each frame */
} gf_frames;

/* Writable column storage for gf_parse_frames (DEVICE pointers, n elements;
 * saddr6/daddr6 16*n bytes, may be NULL to skip IPv6 address extraction). */
typedef struct gf_pkt_cols_out {
    uint16_t *ethertype; uint32_t *saddr4; uint32_t *daddr4; uint8_t *proto;
    int16_t *l4_off; uint32_t *l4w0; uint16_t *l4w3; uint8_t *saddr6; uint8_t *daddr6;
} gf_pkt_cols_out;
int gf_parse_frames(const gf_frames *frames, gf_pkt_cols_out *out, void *stream);

/* ---- XDP prefilter (bpf/bpf_xdp.c, bpf/filter_config.h) ----
 * A zero handle means the corresponding #define is absent. */
typedef struct gf_xdp_cfg {
    int cidr4_hmap;   /* CIDR4_FILTER + CIDR4_HMAP_NAME (v4_fix, HASH, key lpm_v4_key) */
    int cidr4_lmap;   /* CIDR4_LPM_PREFILTER + CIDR4_LMAP_NAME (v4_dyn, LPM_TRIE) */
    int cidr6_hmap;   /* CIDR6_FILTER + v6_fix */
    int cidr6_lmap;   /* CIDR6_LPM_PREFILTER + v6_dyn */
    int lxc_map;      /* cilium_lxc (bpf/lib/maps.h:27-33) */
} gf_xdp_cfg;
int gf_xdp_prog_load(const gf_xdp_cfg *cfg);
/* verdict[i] = GF_XDP_DROP / GF_XDP_PASS. */
int gf_xdp_classify(int prog, const gf_pkt_cols *pkts, uint8_t *verdict, void *stream);

/* bpf_xdp.o as bpf/init.sh attaches it to --prefilter-device (bpf/bpf_xdp.c:158-184), over raw
 * frames: the one program that removes traffic.  Frames in, fewer frames out, in arrival order,
 * as the gf_frames every later frame entry point takes (gf_lb_classify_frames,
 * gf_pipeline_classify, gf_tunnel_decap).
 *
 * verdict[i] is bit for bit what gf_xdp_classify returns for the same frames after
 * gf_parse_frames with the IPv6 columns present: len < 14 drops, IPv4 with len < 34 and IPv6 with
 * len < 54 drop, every other ethertype passes, reads past min(len, snap_stride) see zeros.
 *
 * The j-th row of out->snap is the whole row (snap_stride bytes, verbatim, the bytes past len
 * included) of the j-th XDP_PASS frame in batch order; len[j] is its wire length and index[j] its
 * batch index i, the handle for any side column (flow_hash, tc_index) the caller carries along.
 * The order is stable.  When more than max_out frames pass, the first max_out are written and
 * counts reports both figures: the call is asynchronous and cannot fail late.  Nothing at or past
 * row counts[2] is written in snap, len or index.  There is no in-place mode.
 *
 * The call takes the locks of the program's maps and sees their state at the batch boundary, as
 * gf_xdp_classify does, and the stats sink counts it exactly as gf_xdp_classify would for these
 * frames.  bpf_xdp sends no events: the event ring is not touched.
 *
 * Errors, all before anything is launched or written: -EBADF (not an XDP program), -EFAULT (NULL
 * frames, out or counts; n > 0 with a NULL frames->snap or frames->len; out->snap without
 * out->len), -EINVAL (n > 0 with snap_stride outside 14..256; out->snap NULL with out->len or
 * out->index; an output buffer that overlaps frames->snap or frames->len), -E2BIG (n > 2^30).
 * n == 0 returns 0 and writes only counts (zeros). */
typedef struct gf_xdp_frames_out {
    uint8_t  *verdict;   /* DEVICE, n bytes: GF_XDP_DROP / GF_XDP_PASS per input frame; may be NULL */
    uint8_t  *snap;      /* DEVICE, max_out * frames->snap_stride: the XDP_PASS frames, whole rows,
                            packed in batch order; may be NULL (then len and index must be NULL too) */
    uint32_t *len;       /* DEVICE, max_out: wire length of each packed frame; NULL only with snap NULL */
    uint32_t *index;     /* DEVICE, max_out: batch index i of each packed frame; may be NULL */
    uint32_t  max_out;   /* capacity of snap / len / index in frames */
    uint32_t *counts;    /* DEVICE, 4 words, required: [0] frames passed, [1] frames dropped,
                            [2] frames written = min([0], max_out) (0 with snap NULL), [3] 0 */
} gf_xdp_frames_out;
int gf_xdp_filter_frames(int prog, const gf_frames *frames, const gf_xdp_frames_out *out, void *stream);

/* ---- standalone LB (bpf/bpf_lb.c, bpf/netdev_config.h) ---- */
#define GF_LB_F_L3       (1u << 0)   /* LB_L3 */
#define GF_LB_F_L4       (1u << 1)   /* LB_L4 */
#define GF_LB_F_REDIRECT (1u << 2)   /* LB_REDIRECT defined */
#define GF_LB_F_NO_IPV4  (1u << 3)   /* LB_DISABLE_IPV4 */
#define GF_LB_F_NO_IPV6  (1u << 4)   /* LB_DISABLE_IPV6 */
typedef struct gf_lb_cfg {
    int lb4_services;  /* cilium_lb4_services (key lb4_key 8 B, value lb4_service 12 B) */
    int lb6_services;  /* cilium_lb6_services (key lb6_key 20 B, value lb6_service 24 B) */
    uint32_t flags;
    uint32_t redirect_ifindex; /* LB_REDIRECT */
} gf_lb_cfg;
int gf_lb_prog_load(const gf_lb_cfg *cfg);
/* Output record per packet (12 B). */
typedef struct gf_lb_out {
    uint8_t  action;     /* GF_TC_ACT_OK / SHOT / REDIRECT */
    uint8_t  reason;     /* -DROP_* (or errno for helper failures) when SHOT, else 0 */
    uint16_t slave;      /* selected slave index (0 = not load balanced) */
    uint16_t new_dport;  /* raw be16 destination port after lb*_xlate */
    uint16_t rev_nat;    /* slave's rev_nat_index (raw) */
    uint32_t new_daddr4; /* raw be32 (v4) */
} gf_lb_out;
/* new_daddr6 (16 B per packet, may be NULL) receives the v6 translated address. */
int gf_lb_classify(int prog, const gf_pkt_cols *pkts, gf_lb_out *out,
                   uint8_t *new_daddr6, void *stream);

/* LB_DSTMAC (bpf_lb.c:200-205): the destination MAC written into frames the program
 * redirects.  mac == NULL undefines it.  -EBADF: not an LB program; -EINVAL: the
 * program was loaded without GF_LB_F_REDIRECT (LB_DSTMAC sits inside #ifdef LB_REDIRECT).
 * The reference's eth_store_daddr(skb, mac, 0) cannot fail on a frame long enough to carry an
 * ethertype, and its `ret = DROP_WRITE_ERROR` is overwritten by `return redirect(ifindex, 0)`
 * anyway, so no record ever reports it.  Read by gf_lb_classify_frames only: gf_lb_classify
 * writes no frame, and the LB stage of gf_pipeline_classify does not apply it. */
int gf_lb_prog_set_dstmac(int prog, const uint8_t mac[6]);

/* bpf_lb's from-netdev (bpf_lb.c:169-212) over raw frames: the program as bpf/init.sh:341-342
 * attaches it to the native device of a node in lb mode, where it is the whole datapath.
 * Dispatch on the frame's ethertype (GF_LB_F_NO_IPV4 / _NO_IPV6 and every other ethertype:
 * TC_ACT_OK, frame untouched), handle_ipv4 / handle_ipv6 with revalidate_data (DROP_INVALID),
 * ipv4_hdrlen / ipv6_hdrlen, extract_l4_port under GF_LB_F_L4 (DROP_UNKNOWN_L4 becomes
 * TC_ACT_OK, frame untouched), the service lookup with its L3 fallback, lb*_select_slave with
 * hash = flow_hash[i] (NULL: 0, as gf_pipeline_classify), lb*_lookup_slave (DROP_NO_SERVICE),
 * lb6's new_dst.p4 |= rev_nat_index, then lb4_xlate / lb6_xlate on the frame with the quirks
 * DESIGN.md lists for the pipeline's LB stage, and LB_DSTMAC on the frames it redirects.
 *
 * out[i] and new_daddr6 (16 B per packet, may be NULL) are bit for bit what gf_lb_classify
 * returns for the same packets after gf_parse_frames, the action included: a translated frame is
 * TC_ACT_REDIRECT with GF_LB_F_REDIRECT and TC_ACT_OK without (the record still carries the
 * translation, and the frame is rewritten either way).
 *
 * snap_out: NULL = records only; frames->snap = in place (only the fields the reference writes
 * in a translated frame are stored: dst MAC, IPv4 daddr and header checksum, IPv6 daddr, L4
 * checksum, L4 dport; no other frame is written); any other buffer (n * snap_stride) = every
 * frame, the untouched ones copied verbatim.  snap_stride is gf_pipeline_classify's: 14..256
 * (-EINVAL otherwise), reads past the snap see zeros and writes past it are dropped.
 *
 * With an event ring set, every TC_ACT_SHOT frame appends send_drop_notify_error's record
 * (bpf_lb.c:194-195), byte for byte the one gf_pipeline_classify appends for a frame dropped at
 * GF_STAGE_LB (source, labels and ifindex 0, the captured bytes, the ring-full rule).  bpf_lb
 * sends no trace notification; its cilium_dbg_capture calls (:73, :131, :206, :210) stay out, as
 * on every other frame entry point.  The stats sink counts the call like gf_lb_classify.
 *
 * Errors, all before anything is launched or written: -EBADF (not an LB program), -EFAULT (NULL
 * frames, or n > 0 with a NULL snap, len or out), -EINVAL (snap_stride), -E2BIG (n > 2^30);
 * n == 0 returns 0. */
int gf_lb_classify_frames(int prog, const gf_frames *frames, const uint32_t *flow_hash,
                          gf_lb_out *out, uint8_t *new_daddr6, uint8_t *snap_out, void *stream);

/* ---- endpoint ingress policy (bpf/bpf_lxc.c handle_policy) ---- */
#define GF_LXC_F_DROP_ALL        (1u << 0)  /* DROP_ALL */
#define GF_LXC_F_POLICY_INGRESS  (1u << 1)  /* POLICY_INGRESS */
#define GF_LXC_F_HAVE_L4_POLICY  (1u << 2)  /* HAVE_L4_POLICY */
#define GF_LXC_F_CT_ACCOUNTING   (1u << 3)  /* CONNTRACK_ACCOUNTING */
#define GF_LXC_F_LXC_IPV4        (1u << 4)  /* LXC_IPV4 */
#define GF_LXC_F_POLICY_EGRESS   (1u << 5)  /* POLICY_EGRESS (pkg/endpoint/endpoint.go:153-156, emitted when egress
                                               is enforced, pkg/endpoint/policy.go:820-839) */
#define GF_LXC_F_TRACE_NOTIFY    (1u << 6)  /* TRACE_NOTIFY (pkg/endpoint/endpoint.go:131-134, on by default:
                                               daemon/main.go:629): send_trace_notify records, see below */
#define GF_LXC_F_NO_CONNTRACK    (1u << 7)  /* CONNTRACK undefined: the endpoint's Conntrack option disabled
                                               (pkg/endpoint/endpoint.go:111-114).  Negative sense: a clear bit keeps
                                               conntrack.  ct_lookup / ct_create / ct_delete are the empty stubs of
                                               bpf/lib/conntrack.h:582-617: every packet is CT_NEW, the tuple's ports
                                               stay 0 (the policy lookup uses dport 0), no CT map is read or written.
                                               ct_map4 / ct_map6 may be 0 and are ignored if given; GF_LXC_F_CT_ACCOUNTING
                                               is ignored; n_l4_ingress != 0 or n_l4_egress != 0: -EINVAL
                                               (bpf/lib/l4.h:138-139).  Such programs mix freely with the others in one
                                               array for gf_policy_ingress_classify(_batches) and gf_pipeline_classify.
                                               gf_lxc_egress_classify returns -EOPNOTSUPP for an array that holds one,
                                               before any launch and without touching any state. */
#define GF_LXC_F_DEBUG           (1u << 8)  /* DEBUG with EVENT_SOURCE = LXC_ID: the endpoint's Debug option
                                               (pkg/endpoint/endpoint.go:84,162).  handle_policy's cilium_dbg* messages
                                               go to the event ring, see "debug notifications" below.  Only
                                               gf_policy_ingress_classify and gf_policy_ingress_classify_batches emit
                                               them (IPv4 and IPv6); gf_pipeline_classify*, gf_lxc_egress_classify,
                                               gf_overlay_classify* and gf_host_classify run a program that has the flag
                                               exactly as if it were clear.  Together with GF_LXC_F_NO_CONNTRACK:
                                               gf_lxc_prog_load returns -EOPNOTSUPP before anything is bound.  LB_DEBUG
                                               (the cilium_dbg_lb messages, bpf/lib/lb.h:84-89) is a separate option:
                                               GF_LXC_F_LB_DEBUG. */
#define GF_LXC_F_LB_DEBUG        (1u << 9)  /* LB_DEBUG: the endpoint's DebugLB option (pkg/endpoint/endpoint.go:120-124).
                                               cilium_dbg_lb is cilium_dbg (bpf/lib/lb.h:85-89), which is empty without
                                               DEBUG (bpf/lib/dbg.h:134-233): the flag alone is accepted and the program
                                               runs exactly as without it.  Together with GF_LXC_F_DEBUG,
                                               gf_policy_ingress_classify(_batches) add the reverse-NAT messages of
                                               handle_policy (lb4_rev_nat / lb6_rev_nat, bpf_lxc.c:801-808, 909-918) to
                                               the event ring, see "debug notifications" below; every other entry point
                                               runs the program as if the flag were clear.  With GF_LXC_F_NO_CONNTRACK
                                               it needs no rule of its own (DEBUG | NO_CONNTRACK is refused, and without
                                               DEBUG the flag is inert).  Not built: the cilium_dbg_lb sites of the
                                               from-container section and of bpf_lb (lb4/6_local's service and slave
                                               lookups, DBG_PKT_HASH, the loopback SNAT, the egress lb4/6_rev_nat): no
                                               entry point here sends debug messages for that code. */
#define GF_MAX_L4_INGRESS 64
#define GF_MAX_PORTMAP 16
typedef struct gf_portmap {    /* struct portmap (bpf/lib/common.h), LXC_PORT_MAPPINGS entries */
    uint16_t from;             /* raw be16 */
    uint16_t to;               /* raw be16 */
} gf_portmap;
typedef struct gf_l4_allow {   /* struct l4_allow, bpf/lib/l4.h:126-136 */
    uint16_t port;             /* raw be16 */
    uint16_t proxy;            /* raw be16 */
    uint8_t  nexthdr;
    uint8_t  pad[3];
} gf_l4_allow;
typedef struct gf_lxc_cfg {
    uint32_t lxc_id;           /* LXC_ID */
    uint32_t seclabel;         /* SECLABEL */
    int policy_map;            /* POLICY_MAP (key policy_key 8 B, value policy_entry 24 B) */
    int ct_map4;               /* CT_MAP4 (key ipv4_ct_tuple 14 B, value ct_entry 48 B) */
    int ct_map6;               /* CT_MAP6 (key ipv6_ct_tuple 40 B, value ct_entry 48 B).  Either every
                                  program binds the same map per family (the agent's default,
                                  cilium_ct4_global / cilium_ct6_global) or programs bind maps of their own
                                  (the ConntrackLocal option, cilium_ct4_<id>, pkg/endpoint/bpf.go:268-276),
                                  mixed freely in one array.  With more than one map per family a call runs
                                  the per-endpoint kernels: each packet's program's own map, inserts counted
                                  into that map, the LRU eviction pass on each map after the call.  One map
                                  bound as both a CT_MAP4 and a CT_MAP6: -EINVAL. */
    int cidr4_ingress_map;     /* CIDR4_INGRESS_MAP (LPM_TRIE), 0 = undefined */
    int cidr6_ingress_map;     /* CIDR6_INGRESS_MAP (LPM_TRIE), 0 = undefined */
    int revnat4_map;           /* cilium_lb4_reverse_nat (key u16, value 6 B) */
    int revnat6_map;           /* cilium_lb6_reverse_nat (key u16, value 18 B) */
    uint32_t flags;            /* GF_LXC_F_* */
    uint32_t n_l4_ingress;     /* CFG_L3L4_INGRESS entries */
    gf_l4_allow l4_ingress[GF_MAX_L4_INGRESS];
    /* ---- the from-container section of the same object (bpf_lxc.c:427-738) ---- */
    uint8_t  lxc_mac[6];       /* LXC_MAC (is_valid_lxc_src_mac) */
    uint8_t  node_mac[6];      /* NODE_MAC (is_valid_gw_dst_mac, router MAC of ipv4_l3) */
    uint32_t lxc_ipv4;         /* LXC_IPV4 value (raw be32, is_valid_lxc_src_ipv4) */
    int lb4_services;          /* cilium_lb4_services (LB_L3 + LB_L4: lb4_lookup_service / lb4_local), 0 = none */
    int ipcache_map;           /* cilium_ipcache (endpoint_key 20 B -> remote_endpoint_info 8 B), POLICY_EGRESS */
    int cidr4_egress_map;      /* CIDR4_EGRESS_MAP (LPM_TRIE), 0 = undefined (deny) */
    uint32_t n_portmap;        /* LXC_PORT_MAPPINGS entries (map_lxc_out) */
    gf_portmap portmap[GF_MAX_PORTMAP];
    uint32_t n_l4_egress;      /* CFG_L3L4_EGRESS entries (l4_egress_proxy_lookup) */
    gf_l4_allow l4_egress[GF_MAX_L4_INGRESS];
    uint8_t  lxc_ip6[16];      /* LXC_IP (is_valid_lxc_src_ip) */
    int lb6_services;          /* cilium_lb6_services (lb6_lookup_service / lb6_local), 0 = none */
    int cidr6_egress_map;      /* CIDR6_EGRESS_MAP (LPM_TRIE), 0 = undefined (deny) */
} gf_lxc_cfg;
int gf_lxc_prog_load(const gf_lxc_cfg *cfg);

/* The cilium_policy prog array (bpf/lib/maps.h:36-43): slot lxc_id -> program. */
int gf_policy_array_create(void);
int gf_policy_array_update(int array, uint32_t lxc_id, int prog);  /* prog 0 = delete */

typedef struct gf_node_cfg {   /* node_config.h values used on the path */
    uint32_t host_ifindex;     /* HOST_IFINDEX */
    int      proxy4_map;       /* cilium_proxy4 (proxy4_tbl_key 10 B -> proxy4_tbl_value 16 B), 0 = none */
    int      proxy6_map;       /* cilium_proxy6 (proxy6_tbl_key 22 B -> proxy6_tbl_value 28 B), 0 = none */
    uint32_t ipv4_gateway;     /* IPV4_GATEWAY (raw be32), the proxy redirect's new daddr */
    uint8_t  host_ip6[16];     /* HOST_IP, the IPv6 proxy redirect's new daddr */
    uint8_t  host_mac[6];      /* HOST_IFINDEX_MAC */
    uint8_t  node_mac[6];      /* NODE_MAC */
    /* the from-container path (bpf_lxc.c:427-658) */
    int      lxc_map;          /* cilium_lxc (lookup_ip4_endpoint of the egress path), 0 = none */
    uint32_t ipv4_cluster_range; /* IPV4_CLUSTER_RANGE (raw be32) */
    uint32_t ipv4_cluster_mask;  /* IPV4_CLUSTER_MASK (raw be32) */
    uint32_t ipv4_loopback;    /* IPV4_LOOPBACK (raw be32), lb4_local's loopback SNAT source */
    uint32_t ipv4_mask;        /* IPV4_MASK (raw be32), the tunnel map key of encap_and_redirect */
    uint32_t encap_ifindex;    /* ENCAP_IFINDEX, 0 = undefined (no tunnel) */
    int      tunnel_map;       /* cilium_tunnel_map (endpoint_key 20 B -> endpoint_key 20 B) */
    uint8_t  router_ip6[16];   /* ROUTER_IP (the IPv6 egress path's CLUSTER_ID test) */
} gf_node_cfg;
int gf_node_config(const gf_node_cfg *cfg);

/* Output record per packet (8 B). */
typedef struct gf_ingress_out {
    uint8_t  action;      /* TC_ACT_OK / SHOT / REDIRECT (handle_policy return) */
    uint8_t  reason;      /* cb[2] = -ret when SHOT (bpf/lib/drop.h:92-107) */
    uint8_t  ct_ret;      /* forwarding_reason: CT_NEW/ESTABLISHED/REPLY/RELATED */
    uint8_t  flags;       /* bit0: redirected to proxy, bit1: CT entry created */
    uint16_t proxy_port;  /* raw be16 policy verdict > 0 */
    uint16_t ifindex_lo;  /* low 16 bits of the redirect ifindex */
} gf_ingress_out;
#define GF_INGRESS_F_PROXY    1
#define GF_INGRESS_F_CREATED  2

/* Runs handle_policy over the batch, in batch order per flow group
 * (unordered address pair): packets of one group see each other's CT
 * updates in batch order, as on one CPU of the reference.  now_sec
 * replaces bpf_ktime_get_sec() for the whole batch. */
int gf_policy_ingress_classify(int policy_array, const gf_pkt_cols *pkts,
                               uint32_t now_sec, gf_ingress_out *out, void *stream);
/* nb consecutive gf_policy_ingress_classify calls on `stream` (batch k with
 * now_sec[k] into outs[k]), with identical results.  The stateless half of a
 * batch (record pack, flow-group sort and schedule: no map state) is built on an
 * internal second stream while handle_policy of the previous batch runs, so the
 * schedule leaves the critical path of a stream of batches. */
int gf_policy_ingress_classify_batches(int policy_array, uint32_t nb, const gf_pkt_cols *const *batches,
                                       const uint32_t *now_sec, gf_ingress_out *const *outs, void *stream);

/* ---- endpoint egress: the from-container program (bpf/bpf_lxc.c:685-738
 * handle_ingress -> tail_handle_ipv4 -> handle_ipv4_from_lxc :427-658) ----
 * Frames sent by local endpoints; packet i runs the program of endpoint
 * lxc_id[i] (its bpf_lxc object = the cilium_policy slot's program).  Local
 * deliveries (ipv4_local_delivery, bpf/lib/l3.h:136-168) continue into the
 * destination's handle_policy (tail call into cilium_policy) in a second pass
 * over the batch, as gf_pipeline_classify does: every from-container effect
 * of the batch (CT, proxy map) precedes every handle_policy effect of its
 * deliveries.  IPv6 frames run tail_handle_ipv6 -> ipv6_l3_from_lxc
 * (:120-416).  Frames for the ARP / ICMPv6 responders (tail_handle_arp,
 * icmp6_handle's NS and echo-to-router) are reported as stage GF_STAGE_NONE;
 * gf_respond_calls + gf_respond (below) run those tail calls. */
typedef struct gf_lxc_batch {
    gf_frames frames;          /* DEVICE frames (snap_stride >= every header byte touched, <= 256) */
    const uint16_t *lxc_id;    /* DEVICE: the sending endpoint (whose from-container program runs) */
    const uint32_t *flow_hash; /* DEVICE get_hash_recalc(skb) (lb4_select_slave), may be NULL */
} gf_lxc_batch;
#define GF_STAGE_NONE     0    /* not classified: ARP / ICMPv6 responders (gf_respond) */
#define GF_STAGE_FROM_LXC 5    /* the from-container verdict is final */
/* GF_STAGE_POLICY (4): delivered locally, handle_policy of endpoint lxc_id */
#define GF_EG_F_CREATED   0x0001  /* ct_create4(CT_EGRESS) */
#define GF_EG_F_PROXY     0x0002  /* ipv4_redirect_to_host_port */
#define GF_EG_F_LB        0x0004  /* lb4_local translated the destination */
#define GF_EG_F_LOOPBACK  0x0008  /* ... back to the sender: source SNAT to IPV4_LOOPBACK */
#define GF_EG_F_REVNAT    0x0010  /* lb4_rev_nat of a reply */
#define GF_EG_F_PORTMAP   0x0020  /* map_lxc_out rewrote the source port */
#define GF_EG_F_ENCAP     0x0040  /* encap_and_redirect: tunnel_ip holds the remote node */
#define GF_EG_F_TO_HOST   0x0080  /* to_host: redirect(HOST_IFINDEX) */
#define GF_EG_F_TO_STACK  0x0100  /* pass_to_stack: TC_ACT_OK */
#define GF_EG_F_LOCAL     0x0200  /* ipv4_local_delivery (stage GF_STAGE_POLICY) */
#define GF_EG_F_DELETED   0x0400  /* ct_delete4 of an ESTABLISHED flow the policy now denies */
#define GF_EG_F_ARP       0x0800  /* stage NONE: ARP (tail_handle_arp, the responder) */
#define GF_EG_F_IPV6      0x1000  /* the IPv6 path (ipv6_l3_from_lxc) */
#define GF_EG_F_ICMP6_TE  0x2000  /* hop limit reached in ipv6_l3: icmp6_send_time_exceeded (action
                                     REDIRECT; gf_respond builds the reply, GF_CALL_ICMP6_TIME_EXCEEDED) */
#define GF_EG_F_RESPONDER 0x4000  /* stage NONE: icmp6_handle's NS / echo-to-router responders */
typedef struct gf_egress_out {   /* 24 B; bytes 0-9 as gf_pipeline_out */
    uint8_t  stage;       /* GF_STAGE_FROM_LXC / GF_STAGE_POLICY / GF_STAGE_NONE */
    uint8_t  action;      /* final TC_ACT_* */
    uint8_t  reason;      /* drop reason when SHOT */
    uint8_t  ct_ret;      /* stage FROM_LXC: the egress ct_lookup4 result; POLICY: handle_policy's */
    uint8_t  flags;       /* stage POLICY: gf_ingress_out.flags */
    uint8_t  eg_ct_ret;   /* egress ct_lookup4 result (forwarding_reason) */
    uint16_t proxy_port;  /* raw be16 proxy port of the final redirect */
    uint16_t ifindex_lo;  /* redirect target (HOST_IFINDEX, ENCAP_IFINDEX, or handle_policy's) */
    uint16_t slave;       /* lb4_local: selected slave */
    uint16_t rev_nat;     /* lb4_local: rev_nat_index (raw) */
    uint16_t eg_flags;    /* GF_EG_F_* */
    uint32_t tunnel_ip;   /* ENCAP: bpf_tunnel_key.remote_ipv4 */
    uint16_t lxc_id;      /* stage POLICY: destination endpoint */
    uint16_t pad;
} gf_egress_out;
/* snap_out (n * snap_stride, may be NULL): the frames as the programs left them. */
int gf_lxc_egress_classify(int policy_array, const gf_lxc_batch *batch, uint32_t now_sec,
                           gf_egress_out *out, uint8_t *snap_out, void *stream);

/* ---- full pipeline (BASELINE config 4) ----
 * One frame through the programs a node attaches in order, each seeing the
 * frame as the previous one rewrote it:
 *   bpf_xdp (prefilter)          bpf/bpf_xdp.c:158-184
 *   bpf_lb  from-netdev          bpf/bpf_lb.c:169-212 (lb4_xlate/lb6_xlate rewrites + checksums)
 *   bpf_netdev from-netdev       bpf/bpf_netdev.c:160-247, 326-393 (endpoint lookup,
 *                                ipv{4,6}_local_delivery: TTL/hop limit, MACs, port map)
 *   cilium_policy[ep->lxc_id]    bpf/bpf_lxc.c:980-1024 handle_policy (as gf_policy_ingress_classify)
 * The pipeline replaces the per-program entry points of a node for traffic
 * arriving on the netdev; it has no equivalent call in the reference (the
 * kernel chains the programs), see DESIGN.md. */
#define GF_NETDEV_F_FIXED_SECCTX (1u << 0)  /* FIXED_SRC_SECCTX defined */
#define GF_NETDEV_F_TRACE_NOTIFY (1u << 1)  /* TRACE_NOTIFY: TRACE_FROM_STACK at from_netdev (bpf_netdev.c:436) */
/* The two build options bpf/init.sh gives the native device's object (:179 -DHANDLE_NS always;
 * node_config.h's ENCAP_IFINDEX in tunnel mode, :303-304).  Both are opt-in for the pipeline's
 * netdev stage and ignored by gf_host_load; a pipeline loaded without them is from_netdev compiled
 * without either, whatever gf_node_cfg.encap_ifindex holds.
 *   HANDLE_NS (bpf_netdev.c:180-186, lib/icmp6.h:38-45, 380-401): in handle_ipv6, after ipv6_hdrlen
 *     and before derive_sec_ctx, when the next header ipv6_hdrlen arrived at is ICMPv6 (58; a chain
 *     it rejects leaves ip6->nexthdr, which is never 58): icmp6_handle(skb, ETH_HLEN, ip6).
 *     icmp6_load_type is load_byte (LD_ABS) at the fixed offset 14 + 40 = 54, also behind extension
 *     headers, where byte 54 is the first extension header's own next-header field; a load past the
 *     frame (len 54) ends the program with return value 0 = TC_ACT_OK, the frame untouched and no
 *     notification.  Type 135: the CILIUM_CALL_HANDLE_ICMP6_NS tail call, whatever the target.
 *     Type 128 with ip6->daddr (as bpf_lb left it) == gf_netdev_cfg.router_ip6: the
 *     CILIUM_CALL_SEND_ICMP6_ECHO_REPLY tail call.  Everything else goes on to derive_sec_ctx.
 *     A frame that takes a tail call ends in the front: stage GF_STAGE_NETDEV, action TC_ACT_OK and
 *     reason 0 (as the egress front reports its responders), GF_PIPE_F_RESPONDER, the GF_CALL_* number
 *     in pad0; the frame as bpf_lb left it.  gf_respond_calls + gf_respond run the call (NODE_MAC
 *     from gf_node_config: no lxc_id column).
 *   ENCAP (bpf_netdev.c:225-243, 378-392, lib/encap.h:30-70): after the cilium_lxc lookup missed,
 *     the cluster-range test and encap_and_redirect of gf_host_classify (below), with secctx =
 *     derive_sec_ctx / derive_ipv4_sec_ctx / FIXED_SRC_SECCTX; a tunnel-map miss falls through to
 *     TC_ACT_OK.  Record: stage GF_STAGE_NETDEV, action REDIRECT, ifindex_lo = ENCAP_IFINDEX,
 *     GF_PIPE_F_ENCAP; the tunnel endpoint goes to gf_pipeline_classify_tunnel's tunnel_ip column
 *     (daddr4 keeps lb4_xlate's address).  With GF_NETDEV_F_TRACE_NOTIFY the redirect appends
 *     TRACE_TO_OVERLAY (src_label = secctx, ifindex = ENCAP_IFINDEX) after TRACE_FROM_STACK.
 *     gf_pipeline_load: -EINVAL unless gf_node_cfg.encap_ifindex != 0 and a tunnel map is set. */
#define GF_NETDEV_F_HANDLE_NS    (1u << 2)  /* HANDLE_NS defined */
#define GF_NETDEV_F_ENCAP        (1u << 3)  /* ENCAP_IFINDEX defined (= gf_node_cfg.encap_ifindex) */
typedef struct gf_netdev_cfg {
    int lxc_map;               /* cilium_lxc (endpoint_key 20 B -> endpoint_info 112 B) */
    uint32_t flags;            /* GF_NETDEV_F_* */
    uint32_t fixed_secctx;     /* FIXED_SRC_SECCTX */
    uint8_t  router_ip6[16];   /* ROUTER_IP (node_config.h), derive_sec_ctx() */
    uint32_t ingress_ifindex;  /* skb->ingress_ifindex of the frames (the netdev's ifindex) */
} gf_netdev_cfg;
typedef struct gf_pipeline_cfg {
    int xdp_prog;              /* gf_xdp_prog_load handle, 0 = no XDP program attached */
    int lb_prog;               /* gf_lb_prog_load handle, 0 = no LB program attached */
    gf_netdev_cfg netdev;
    int policy_array;          /* cilium_policy prog array */
} gf_pipeline_cfg;
int gf_pipeline_load(const gf_pipeline_cfg *cfg);

typedef struct gf_pipe_batch {
    gf_frames frames;          /* DEVICE frames; snap_stride must hold every header byte the
                                  programs read or write (>= l4_off + 18) */
    const uint8_t  *tc_index;  /* skb->tc_index (DEVICE, may be NULL) */
    const uint32_t *flow_hash; /* get_hash_recalc(skb) (DEVICE, may be NULL) */
} gf_pipe_batch;

#define GF_STAGE_XDP    1      /* dropped by bpf_xdp (action = XDP_DROP) */
#define GF_STAGE_LB     2      /* bpf_lb verdict is final (SHOT, or REDIRECT with LB_REDIRECT) */
#define GF_STAGE_NETDEV 3      /* bpf_netdev verdict is final (to the stack, SHOT, ICMPv6 reply) */
#define GF_STAGE_POLICY 4      /* tail-called into cilium_policy: handle_policy's verdict */
#define GF_PIPE_F_RESPONDER 0x04  /* stage NETDEV, GF_NETDEV_F_HANDLE_NS: icmp6_handle took a responder tail call (pad0) */
#define GF_PIPE_F_ENCAP     0x08  /* stage NETDEV, GF_NETDEV_F_ENCAP: encap_and_redirect (tunnel_ip column) */
#define GF_PIPE_F_ICMP6_TE  0x20  /* hop limit reached: icmp6_send_time_exceeded (bpf/lib/icmp6.h:313-322);
                                     action REDIRECT; gf_respond builds the reply (GF_CALL_ICMP6_TIME_EXCEEDED) */
#define GF_PIPE_F_LB        0x40  /* translated by lb*_xlate */
#define GF_PIPE_F_PORTMAP   0x80  /* dport rewritten by map_lxc_in */
typedef struct gf_pipeline_out {   /* 24 B */
    uint8_t  stage;       /* GF_STAGE_* */
    uint8_t  action;      /* XDP_DROP at stage XDP, else TC_ACT_* */
    uint8_t  reason;      /* drop reason (cb[2]) when SHOT */
    uint8_t  ct_ret;      /* stage POLICY: CT_NEW/ESTABLISHED/REPLY/RELATED */
    uint8_t  flags;       /* gf_ingress_out.flags | GF_PIPE_F_* */
    uint8_t  pad0;        /* GF_PIPE_F_RESPONDER: the GF_CALL_* tail call taken; else 0 */
    uint16_t proxy_port;  /* stage POLICY: raw be16 */
    uint16_t ifindex_lo;  /* redirect target (LB_REDIRECT ifindex, or handle_policy's) */
    uint16_t slave;       /* LB: selected slave */
    uint16_t rev_nat;     /* LB: slave's rev_nat_index */
    uint16_t dport;       /* raw be16 dport written by lb*_xlate / map_lxc_in (0 = unchanged) */
    uint32_t daddr4;      /* raw be32 daddr written by lb4_xlate (0 = unchanged) */
    uint16_t lxc_id;      /* stage POLICY: endpoint tail-called into */
    uint16_t pad1;
} gf_pipeline_out;
/* new_daddr6 (16 B per packet, may be NULL): lb6_xlate's address.  snap_out
 * (n * snap_stride, may be NULL): every frame as rewritten before handle_policy
 * (MACs, TTL/hop limit, daddr, dport, IPv4 + L4 checksums). */
int gf_pipeline_classify(int pipe, const gf_pipe_batch *batch, uint32_t now_sec, gf_pipeline_out *out,
                         uint8_t *new_daddr6, uint8_t *snap_out, void *stream);
/* gf_pipeline_classify with one more optional column: tunnel_ip (DEVICE, n u32, may be NULL) =
 * bpf_tunnel_key.remote_ipv4 of the frames that took GF_NETDEV_F_ENCAP's redirect, host byte order
 * as gf_egress_out.tunnel_ip, 0 for every other frame.  A frame load-balanced to a backend on
 * another node has both daddr4 and tunnel_ip.  gf_pipeline_classify forwards here with NULL. */
int gf_pipeline_classify_tunnel(int pipe, const gf_pipe_batch *batch, uint32_t now_sec, gf_pipeline_out *out,
                                uint8_t *new_daddr6, uint8_t *snap_out, uint32_t *tunnel_ip, void *stream);

/* ---- from-overlay: the program on the tunnel device (bpf/bpf_overlay.c:38-200) ----
 * In tunnel mode every cross-node pod-to-pod packet reaches its endpoint
 * through this program: the frames gf_lxc_egress_classify reports with
 * GF_EG_F_ENCAP on the sending node, as the VXLAN device hands their inner
 * frame to tc on the receiving one, with bpf_tunnel_key.tunnel_id = the
 * sender's security identity.  ENCAP_GENEVE undefined, ENABLE_IPV4 defined.
 *   0x0800: len < 34 DROP_INVALID; lookup_ip4_endpoint(daddr) in cilium_lxc:
 *           no entry DROP_NON_LOCAL; ENDPOINT_F_HOST -> to_host: ipv4_l3(NODE_MAC,
 *           HOST_IFINDEX_MAC) (TTL <= 1 DROP_INVALID) and redirect(HOST_IFINDEX), or
 *           TC_ACT_OK with the frame untouched when HOST_IFINDEX is undefined
 *           (gf_node_cfg.host_ifindex == 0); else ipv4_local_delivery with
 *           seclabel = tunnel_id and the cilium_policy tail call
 *   0x86DD: len < 54 DROP_INVALID; the same three outcomes with ipv6_l3 (hop limit
 *           <= 1: icmp6_send_time_exceeded, reported as action REDIRECT with
 *           GF_PIPE_F_ICMP6_TE) and ipv6_local_delivery; no icmp6_handle, no
 *           derive_sec_ctx
 *   other:  TC_ACT_OK
 * Errors end in send_drop_notify_error(skb, ret, TC_ACT_SHOT).  Not modelled:
 * skb_get_tunnel_key failing (DROP_NO_TUNNEL_KEY: it cannot for a frame received
 * from the tunnel device).  Geneve tunnel mode: GF_OVERLAY_F_GENEVE (at the end of this header).
 * Records are gf_pipeline_out: stage GF_STAGE_OVERLAY for the verdicts the program
 * itself ends (to_host: action REDIRECT, ifindex_lo = HOST_IFINDEX), stage
 * GF_STAGE_POLICY for tail-called packets, completed by handle_policy as in the
 * pipeline (lxc_id, ct_ret, flags, proxy_port, ifindex_lo, GF_PIPE_F_PORTMAP with
 * dport); slave, rev_nat and daddr4 stay 0.  HOST_IFINDEX, HOST_IFINDEX_MAC and
 * NODE_MAC come from gf_node_config.  With an event ring set, drops are recorded as
 * the pipeline records them and GF_OVERLAY_F_TRACE_NOTIFY makes each packet's first
 * record TRACE_FROM_OVERLAY (subtype 9, ifindex = ingress_ifindex, the frame as
 * received; bpf_overlay.c:174). */
#define GF_DROP_NON_LOCAL 151      /* DROP_NON_LOCAL, bpf/lib/common.h:245 */
#define GF_STAGE_OVERLAY  6        /* the from-overlay verdict is final */
#define GF_OVERLAY_F_TRACE_NOTIFY (1u << 0)
typedef struct gf_overlay_cfg {
    int lxc_map;                   /* cilium_lxc */
    uint32_t flags;                /* GF_OVERLAY_F_* */
    uint32_t ingress_ifindex;      /* the tunnel device's ifindex (TRACE_FROM_OVERLAY) */
    int policy_array;              /* cilium_policy prog array */
} gf_overlay_cfg;
int gf_overlay_load(const gf_overlay_cfg *cfg);
typedef struct gf_overlay_batch {
    gf_frames frames;              /* DEVICE inner frames, snap_stride 14..256 as the pipeline */
    const uint32_t *tunnel_id;     /* DEVICE, bpf_tunnel_key.tunnel_id per frame; required */
    const uint8_t  *tc_index;      /* DEVICE, may be NULL */
    const uint32_t *flow_hash;     /* DEVICE, may be NULL (the event records' hash) */
} gf_overlay_batch;
/* snap_out (n * snap_stride, may be NULL): every frame as rewritten before
 * handle_policy.  -EBADF, -EFAULT (a NULL batch, frame pointer, out or tunnel_id),
 * -EINVAL (snap_stride < 14 or > 256), -E2BIG; n == 0 returns 0. */
int gf_overlay_classify(int ovl, const gf_overlay_batch *batch, uint32_t now_sec,
                        gf_pipeline_out *out, uint8_t *snap_out, void *stream);

/* ---- from-host: the program on cilium_host (bpf/bpf_netdev.c:50-468 compiled with
 * -DFROM_HOST, bpf/init.sh:359-360) ----
 * Everything the host sends to pods takes this program: health probes, kubelet, host
 * to remote pods over the tunnel, and the L7 proxy's return path, which is where the
 * cilium_proxy{4,6} entries handle_policy and the container egress path write are
 * read back.  FROM_HOST and ENABLE_IPV4 defined, HANDLE_NS undefined (no responders),
 * FIXED_SRC_SECCTX per gf_netdev_cfg, ENCAP_IFINDEX defined iff
 * gf_node_cfg.encap_ifindex != 0.  Per frame, in the reference's order:
 *   from_netdev (:414-468): handle_identity_from_proxy (:128-145) on mark:
 *           mark & 0xFFF == 0xFEA (ingress proxy): proxy_identity = mark >> 16 and
 *           tc_index |= TC_INDEX_F_SKIP_PROXY; == 0xFEB (egress proxy): proxy_identity
 *           only; else neither.  The reset of skb->mark to 0 has no output column.
 *           Ethertype other than 0x0800 / 0x86DD: TC_ACT_OK, frame untouched.
 *   handle_ipv4 (:328-396) / handle_ipv6 (:163-246): len < 34 / 54 DROP_INVALID;
 *           secctx = FIXED_SRC_SECCTX, else WORLD_ID (v4) / derive_sec_ctx (v6),
 *           overridden by a non-zero proxy_identity;
 *           reverse_proxy (:264-325) / reverse_proxy6 (:67-124), TCP and UDP only (v6:
 *           by ip6->nexthdr, so a frame with an extension header is ignored): the 4 port
 *           bytes not loadable DROP_CT_INVALID_HDR; key {saddr = daddr, dport = sport,
 *           sport = dport, nexthdr} in cilium_proxy4 / 6 (lifetime is not consulted); on
 *           a hit l4_modify_port of the source port (its checksum field outside the frame:
 *           DROP_WRITE_ERROR), the source address, the IPv4 header checksum, the L4
 *           checksum (BPF_F_PSEUDO_HDR; UDP with BPF_F_MARK_MANGLED_0), tc_index |=
 *           TC_INDEX_F_SKIP_PROXY, and GF_PIPE_F_REV_PROXY in the record;
 *           rewrite_dmac_to_host (:148-160): dmac = CILIUM_NET_MAC, hit or miss;
 *           the endpoint lookup in cilium_lxc: ENDPOINT_F_HOST TC_ACT_OK; a local
 *           endpoint ipv{4,6}_local_delivery with secctx (TTL <= 1 DROP_INVALID, hop
 *           limit <= 1 GF_PIPE_F_ICMP6_TE) and the cilium_policy tail call; no endpoint,
 *           ENCAP_IFINDEX defined and the destination in the cluster range (v4:
 *           ipv4_cluster_mask / range; v6: the /96 of gf_node_cfg.router_ip6):
 *           encap_and_redirect (lib/encap.h:30-70) with the tunnel_map key daddr &
 *           ipv4_mask (v6: daddr/96), a miss falling through; otherwise TC_ACT_OK.
 * Errors end in send_drop_notify_error(skb, ret, TC_ACT_SHOT).
 * Records are gf_pipeline_out: stage GF_STAGE_HOST for the verdicts the program itself
 * ends; an encap redirect has action REDIRECT, ifindex_lo = ENCAP_IFINDEX and, reusing
 * the field lb4_xlate's address has in the pipeline, daddr4 = the tunnel endpoint
 * (bpf_tunnel_key.remote_ipv4, host byte order as gf_egress_out.tunnel_ip).  Tail-called
 * packets get stage GF_STAGE_POLICY, completed by handle_policy as for the overlay.
 * GF_PIPE_F_REV_PROXY lies outside the three flag bits the pipeline's front hands
 * handle_policy in gf_rec.cls; it is carried in the record itself, which handle_policy
 * completes by read-modify-write for this entry point.
 * Ordering: the front reads cilium_proxy4 / 6 as they stood when the call began; a
 * reverse lookup never sees an entry handle_policy creates later in the same call.  The
 * call holds the maps' locks from before the front's reads to after handle_policy's
 * writes.  The proxy maps, tunnel map, cluster values and encap_ifindex come from
 * gf_node_config.  With an event ring set, drops are recorded as the pipeline records
 * them and GF_NETDEV_F_TRACE_NOTIFY makes each packet's first record TRACE_FROM_PROXY
 * (subtype 6, src_label = proxy_identity) when proxy_identity != 0, else TRACE_FROM_HOST
 * (subtype 7, src_label = HOST_ID); ifindex = ingress_ifindex, the frame as received
 * (:423-433).  A mark of 0x00000FEA sets the skip bit but leaves proxy_identity 0, so it
 * traces as FROM_HOST.  An encap redirect adds TRACE_TO_OVERLAY (src_label = secctx,
 * ifindex = ENCAP_IFINDEX). */
#define GF_STAGE_HOST 7            /* the from-host verdict is final */
#define GF_PIPE_F_REV_PROXY 0x10   /* gf_pipeline_out.flags: reverse_proxy / reverse_proxy6 translated the source */
typedef struct gf_host_cfg {
    gf_netdev_cfg netdev;          /* lxc_map, GF_NETDEV_F_FIXED_SECCTX / _TRACE_NOTIFY, fixed_secctx,
                                      router_ip6 (derive_sec_ctx), ingress_ifindex (cilium_host's) */
    uint8_t cilium_net_mac[6];     /* CILIUM_NET_MAC (rewrite_dmac_to_host) */
    int policy_array;              /* cilium_policy prog array */
} gf_host_cfg;
int gf_host_load(const gf_host_cfg *cfg);
typedef struct gf_host_batch {
    gf_frames frames;              /* DEVICE frames, snap_stride 14..256 as the pipeline */
    const uint32_t *mark;          /* DEVICE skb->mark per frame; may be NULL (all 0) */
    const uint8_t  *tc_index;      /* DEVICE, may be NULL */
    const uint32_t *flow_hash;     /* DEVICE, may be NULL (the event records' hash) */
} gf_host_batch;
/* snap_out (n * snap_stride, may be NULL): every frame as rewritten before
 * handle_policy.  -EBADF, -EFAULT (a NULL batch, frame pointer or out), -EINVAL
 * (snap_stride < 14 or > 256), -E2BIG; n == 0 returns 0. */
int gf_host_classify(int host, const gf_host_batch *batch, uint32_t now_sec,
                     gf_pipeline_out *out, uint8_t *snap_out, void *stream);

/* ---- ARP and ICMPv6 responders: the reply frames, built on the device ----
 * The four responder tail calls of the reference, run after a classify call over
 * the frames it reported for them:
 *   egress records   GF_STAGE_NONE + GF_EG_F_ARP         -> GF_CALL_ARP
 *                    GF_STAGE_NONE + GF_EG_F_RESPONDER   -> GF_CALL_ICMP6_NS (ICMPv6 type 135) /
 *                                                           GF_CALL_ICMP6_ECHO_REPLY
 *                    GF_EG_F_ICMP6_TE                    -> GF_CALL_ICMP6_TIME_EXCEEDED
 *   pipeline, overlay and from-host records GF_PIPE_F_ICMP6_TE -> GF_CALL_ICMP6_TIME_EXCEEDED
 *   pipeline records GF_PIPE_F_RESPONDER (GF_NETDEV_F_HANDLE_NS) -> the record's pad0: GF_CALL_ICMP6_NS /
 *                                                           GF_CALL_ICMP6_ECHO_REPLY (the frame is not read)
 * nh_off is ETH_HLEN at every call site.  IPV4_GATEWAY and ROUTER_IP come from
 * gf_node_config; NODE_MAC from the program in slot lxc_id[i] of the responder's
 * cilium_policy array (gf_lxc_cfg.node_mac), or from gf_node_cfg.node_mac when the
 * batch has no lxc_id column.
 *   ARP (arp_respond): len < 42 TC_ACT_OK; a request (ar_op 1, ar_hrd 1) to the broadcast
 *     address or NODE_MAC for IPV4_GATEWAY is answered in place (action REDIRECT);
 *     anything else TC_ACT_OK, untouched.  DROP_ALL endpoints answer too.
 *   NS (__icmp6_handle_ns): target (bytes 62..78) unreadable DROP_INVALID; not ROUTER_IP
 *     DROP_UNKNOWN_TARGET (TC_ACT_OK under GF_RESPOND_F_NS_TO_STACK); else a neighbour
 *     advertisement (type 136, router + solicited, target link-layer option NODE_MAC;
 *     option bytes 78..86 unreadable: DROP_INVALID after the header was rewritten).
 *   ECHO_REPLY (__icmp6_send_echo_reply): type 129, identifier and sequence kept.  The
 *     daddr == ROUTER_IP test belongs to the caller (icmp6_handle) and is not repeated.
 *   TIME_EXCEEDED (__icmp6_send_time_exceeded, HAVE_SKB_CHANGE_TAIL): embeds the IPv6
 *     header and 8 (ICMPv6, UDP) or 20 (TCP) upper bytes; other next headers
 *     DROP_UNKNOWN_L4, unreadable upper bytes DROP_INVALID (both after nexthdr was set to 58);
 *     new_len = len + 56|68 - ntohs(payload_len) in u32; < 54 or > max_len DROP_WRITE_ERROR
 *     (skb_change_tail), as is a payload that no longer fits new_len.  Growth is zero-filled.
 *   The three ICMPv6 calls end in icmp6_send_reply: saddr = ROUTER_IP, daddr = old saddr,
 *     dmac = old smac, smac = NODE_MAC, the checksum adjusted by csum_diff, action REDIRECT
 *     (back out skb->ifindex, which has no output column).
 * Incremental checksum updates keep a wrong request checksum wrong, as the reference does.
 * A frame that fails midway keeps its partial rewrites in snap_out.  With an event ring
 * set every SHOT appends one drop record (send_drop_notify_error: labels, dst_id and
 * ifindex 0; source = LXC_ID of the calling endpoint's program, 0 for the node's; len_orig
 * the length at the error; the payload the frame as it stood then).  The responders send
 * no trace records.  Missed tail calls: a call value above 4, or an lxc_id whose slot holds
 * no program (every slot, for a responder without a policy array): SHOT with
 * GF_DROP_MISSED_TAIL_CALL, the frame's row in snap_out not written.  Call 0: the record is
 * {OK, 0, 0, 0, len} and the row in snap_out is not written (the caller's bytes stay). */
#define GF_CALL_NONE                 0
#define GF_CALL_ARP                  1  /* tail_handle_arp            bpf/bpf_lxc.c:692-696, lib/arp.h:34-95 */
#define GF_CALL_ICMP6_NS             2  /* tail_icmp6_handle_ns       lib/icmp6.h:146-199, 331-361 */
#define GF_CALL_ICMP6_ECHO_REPLY     3  /* tail_icmp6_send_echo_reply lib/icmp6.h:84-127 */
#define GF_CALL_ICMP6_TIME_EXCEEDED  4  /* tail_icmp6_send_time_exceeded lib/icmp6.h:201-312 (HAVE_SKB_CHANGE_TAIL) */
#define GF_DROP_UNKNOWN_TARGET 150      /* bpf/lib/common.h:244 */

#define GF_RESPOND_F_NS_TO_STACK (1u << 0) /* ACTION_UNKNOWN_ICMP6_NS = TC_ACT_OK (bpf_netdev.c:25);
                                              clear: DROP_UNKNOWN_TARGET (icmp6.h:34-36, the bpf_lxc build) */
typedef struct gf_respond_cfg {
    int      policy_array;  /* NODE_MAC of the calling endpoint's program; 0 = none */
    uint32_t flags;         /* GF_RESPOND_F_* (other bits: -EINVAL) */
    uint32_t max_len;       /* skb_change_tail's upper bound (dev->mtu + hard_header_len); 0 = 1514 */
} gf_respond_cfg;
int gf_respond_load(const gf_respond_cfg *cfg);

typedef struct gf_respond_batch {
    gf_frames       frames;    /* DEVICE; each frame as it stood at the tail call */
    const uint8_t  *call;      /* DEVICE, GF_CALL_* per frame; required */
    const uint16_t *lxc_id;    /* DEVICE, the endpoint whose object makes the call; NULL = the node's
                                  programs (NODE_MAC from gf_node_config) */
    const uint32_t *flow_hash; /* DEVICE, may be NULL (drop records' hash) */
} gf_respond_batch;
typedef struct gf_respond_out {   /* 8 B */
    uint8_t  action;   /* TC_ACT_REDIRECT = the reply goes back out skb->ifindex; OK; SHOT */
    uint8_t  reason;   /* -DROP_* when SHOT */
    uint8_t  call;     /* the call that ran (echo of the column) */
    uint8_t  pad;
    uint32_t len;      /* skb->len after the call (changes only for TIME_EXCEEDED) */
} gf_respond_out;
/* snap_out (n * snap_stride, required, not frames.snap): the rows of the frames with a call, as
 * the call left them; bytes of a TIME_EXCEEDED row at or past the new length are 0.
 * -EBADF (not a responder handle), -EFAULT (a NULL batch, frame pointer, call, out or snap_out),
 * -EINVAL (snap_stride outside 122..256 = 14 + 40 + 68, the furthest byte a call touches;
 * snap_out == frames.snap), -E2BIG; n == 0 returns 0.  Every refusal precedes any launch. */
int gf_respond(int resp, const gf_respond_batch *batch, gf_respond_out *out, uint8_t *snap_out, void *stream);

#define GF_REC_EGRESS   1   /* gf_egress_out  */
#define GF_REC_PIPELINE 2   /* gf_pipeline_out (pipeline, overlay, from-host) */
/* call[i] (DEVICE, n bytes) from the records of a classify call over `frames`, by the table above;
 * everything else GF_CALL_NONE.  -EFAULT, -EINVAL (rec_kind), -E2BIG; n == 0 returns 0. */
int gf_respond_calls(const gf_frames *frames, const void *records, uint32_t rec_kind, uint8_t *call, void *stream);

/* ---- ingest re-partition for N GPUs (real traffic) ----
 * owner[i] = the rank owning packet i's flow group: the unordered address pair
 * handle_policy's conntrack sees (after bpf_lb's translation, which is
 * stateless), fmix64-hashed mod nranks (frames that cannot reach conntrack
 * stay on self_rank); order = the packet indices stably grouped by owner;
 * counts[r] = packets for rank r.  All DEVICE pointers (n, n, nranks
 * elements).  The caller exchanges the frames (cilium_amd.shard: one RCCL
 * all-to-all) and classifies what it receives. */
int gf_pipeline_partition(int pipe, const gf_pipe_batch *batch, uint32_t self_rank, uint32_t nranks,
                          uint32_t *owner, uint32_t *order, uint32_t *counts, void *stream);

/* ---- conntrack garbage collection ----
 * ctmap.GC(m, name, GCFilterByTime) / ctmap.Flush (pkg/maps/ctmap/ctmap.go:277-368):
 * deletes every entry of a CT map (key ipv4_ct_tuple 14 B or ipv6_ct_tuple 40 B,
 * value ct_entry 48 B) whose lifetime < filter_time (Flush: 0xFFFFFFFF) and
 * returns how many were deleted (or -errno).  Runs on the device replica when the
 * datapath owns the map (compacting probe clusters in the same sweep), else on the
 * host shadow.  Synchronous on `stream`. */
int gf_ct_gc(int map, uint32_t filter_time, void *stream);
/* One GC round over many CT maps in one call: an iteration of the agent's loop
 * (EnableConntrackGC, pkg/endpointmanager/conntrack.go:84-130), which every 10 s collects
 * each endpoint's local cilium_ct4_<id> / cilium_ct6_<id> (the ConntrackLocal option) and the
 * global pair once.  The outcome is exactly that of gf_ct_gc(maps[k], filter_time, stream)
 * for k = 0..n-1: entries with lifetime < filter_time deleted (0xFFFFFFFF: Flush), probe
 * clusters compacted, every swept map's element count exact afterwards (a HASH map that was
 * full takes inserts again).  deleted[k] (host memory, n entries, may be NULL) receives map
 * k's count; the return value is their sum capped at 0x7fffffff, or -errno.  IPv4 and IPv6
 * maps, LRU_HASH and HASH maps and both value layouts mix in one array.  A map whose host
 * shadow is authoritative is collected there, one that never materialised counts 0 (a call
 * over such maps only launches nothing and needs no device); the device-owned maps are swept
 * together, 32 per chain of launches whose grid covers all their slots, their counts fixed
 * on the device, with one readback of all results and one synchronise for the call.
 * Refused before any map is touched or anything is launched: -EFAULT (maps == NULL with
 * n > 0), -EBADF (a handle that is not a map), -EINVAL (a map gf_ct_gc refuses: proxy, LPM
 * and other non-CT maps; or the same map object twice, a second handle from gf_obj_get
 * included), -E2BIG (n > 65536).  n == 0 returns 0.  Locks every map for the call (address
 * order, as the classify calls) and is ordered against the calls that use any of them on
 * other streams.  Synchronous on `stream`. */
int gf_ct_gc_maps(const int *maps, uint32_t n, uint32_t filter_time,
                  uint32_t *deleted /* n entries, host memory, may be NULL */, void *stream);

/* ---- proxy map garbage collection and redirect-close cleanup ----
 * For cilium_proxy4 / cilium_proxy6: hash maps with key/value sizes 10/16
 * (proxy4_tbl_key / proxy4_tbl_value) or 22/28 (the v6 pair, bpf/lib/common.h:445-475);
 * anything else is -EINVAL (gf_ct_gc in turn refuses these maps), a handle that is not a
 * map -EBADF.  Both run on the host shadow while it is authoritative (no device needed),
 * else as a sweep of the device replica that compacts the probe clusters it empties, with
 * no whole-table transfer; afterwards the map's element count is exact again, on the
 * device and in the host's bound of it, so that later classify calls apply their proxy
 * updates in parallel whenever count + updates <= max_entries.  Synchronous on `stream`,
 * ordered against the classify calls that use the map on other streams. */
/* proxymap.GC / Flush (pkg/maps/proxymap/ipv4.go:136-171, ipv6.go): delete every entry with
 * value.lifetime < filter_time (strict: lifetime == filter_time stays).  Returns the number
 * deleted (capped at 0x7fffffff) or -errno.  Flush in the reference is gc(math.MaxUint64),
 * whose uint32(time / 1e9) is 1266874889, not 0xFFFFFFFF; this call takes any u32. */
int gf_proxy_gc(int map, uint32_t filter_time, void *stream);
/* cleanupIPv4Redirects / cleanupIPv6Redirects (ipv4.go:173-195): delete every entry whose
 * key.dport == dport (raw be16, as stored) and key.nexthdr == 6.  Returns the number deleted. */
int gf_proxy_cleanup_port(int map, uint16_t dport, void *stream);

/* ---- LRU CT maps (BPF_MAP_TYPE_LRU_HASH, bpf/bpf_lxc.c:53-75) ----
 * The kernel evicts from per-CPU LRU lists (the tail of an inactive list kept
 * about as long as the active one) in a nondeterministic order and never fails
 * an insert.  libgpuflow's deterministic stand-in: inside a batch an
 * LRU CT map may exceed max_entries (up to the 7/8 load of its slot array: a power
 * of two >= 8 x max_entries for ipv4_ct_tuple, 4 x for ipv6_ct_tuple).  At the end
 * of every classify call that uses it, once the count exceeds the high-water mark
 * HW = max_entries - max_entries/8, a hand sweeping the table's home lines deletes
 * the entries of the older half (age key <= age_cut: the median age of a sample —
 * the max(65536, lines/1024) home lines just ahead of the hand, or the whole table if
 * no entry is homed there; closing entries older than all others, then by last use
 * in one-second bins) homed in the lines it passes, as many lines as bring the count
 * back to HW by the sample's density.  A map running at HW so deletes in each call
 * about what the call inserted: the eviction's work per call follows the call's
 * inserts, not the table.  If the count is still above max_entries, a second round
 * passes more lines by the same estimate and a third the rest of the table.
 * Bound: after a call the count is <= max_entries unless the whole table held
 * fewer than count - max_entries entries of the sample's older half (a single call
 * inserting more than about half of max_entries beyond HW); it never falls below
 * the entries younger than age_cut.  Every eviction is logged: */
typedef struct gf_ct_evict_rec {
    uint32_t seq;              /* the map's classify call (1 = first call that used the map) */
    uint32_t now_sec;          /* that call's now_sec */
    uint32_t age_cut;          /* entries with age key <= age_cut were eligible */
    uint32_t pad;
    uint64_t hand_line;        /* the first home line the hand passed */
    uint64_t lines;            /* home lines passed (from hand_line, wrapping) */
    uint64_t evicted;          /* entries deleted */
} gf_ct_evict_rec;
/* Copies up to max records (oldest first) and returns the number logged. */
int gf_ct_evict_log(int map, gf_ct_evict_rec *out, uint32_t max);
/* Element accounting of a classify call.  Each CT map has an insert limit: the 7/8 load of
 * the slot array for an LRU CT map (7168 for an ipv4_ct_tuple map of max_entries 700,
 * 458752 for one of 64000, 229376 for an ipv6_ct_tuple map of 64000), max_entries for a
 * HASH map.  A pass over n packets is charged per_pkt x n inserts: 2 for handle_policy
 * (ingress, the pipeline, the deliveries of the other entry points), 3 for the
 * from-container pass.  While the host's upper bound of the map's count plus that charge
 * stays within the limit, lanes insert freely and add their net inserts to the count
 * afterwards.  Otherwise (after the bound was tightened from the last eviction's count,
 * or read back when the charge alone fits) the family counts every insert exactly, with
 * an atomic on the count per insert, so that a HASH map fails at exactly max_entries and
 * an LRU map never overruns its slot array.  An egress batch with an exactly counted
 * family runs one packet at a time; in a handle_policy pass a family with a HASH map over
 * its limit runs as one flow group, in batch order, so that the insert that finds the map
 * full is the one that would in the reference.
 * With per-endpoint maps (ConntrackLocal) every map of a family is charged the whole
 * batch, not the packets of its own endpoint, and one map over its limit makes the
 * family exact for the call.  With the reference's 64000-entry local maps this happens to
 * an egress batch of more than 458752 / 3 = 152917 packets (LRU; 229376 / 3 = 76458 for
 * the IPv6 maps) or 64000 / 3 = 21333 packets (HASH) even on empty maps; its deliveries'
 * handle_policy, charged 2n on top of the 3n, first waits for the device's count from
 * 458752 / 5 = 91750 (12800) packets on.  Records stay exact; throughput does not. */

/* ---- drop notifications (bpf/lib/drop.h:38-107, DROP_NOTIFY) ----
 * With a ring set, gf_policy_ingress_classify and gf_pipeline_classify append
 * one record per dropped packet (TC_ACT_SHOT; XDP drops send none), in batch
 * order: struct drop_notify (32 B: type CILIUM_NOTIFY_DROP=1, subtype = drop
 * reason, source = EVENT_SOURCE, hash, len_orig, len_cap, src_label, dst_label,
 * dst_id, ifindex — the layout pkg/monitor/datapath_drop.go DropNotify decodes)
 * followed by GF_TRACE_PAYLOAD_LEN bytes holding the first len_cap bytes of the
 * frame (the pipeline's frames; zeros for column batches, which carry none).
 * *count accumulates across calls; records past `capacity` are lost (a perf ring
 * overrun). */
/* ---- trace notifications (bpf/lib/trace.h:59-106, TRACE_NOTIFY) ----
 * Programs loaded with GF_LXC_F_TRACE_NOTIFY (and a pipeline whose netdev has
 * GF_NETDEV_F_TRACE_NOTIFY) also append struct trace_notify records to the same
 * ring (type CILIUM_NOTIFY_TRACE=4, subtype = observation point TRACE_TO_LXC 0,
 * TO_PROXY 1, TO_HOST 2, TO_STACK 3, TO_OVERLAY 4, FROM_LXC 5, FROM_STACK 8, FROM_OVERLAY 9
 * (gf_overlay_classify with GF_OVERLAY_F_TRACE_NOTIFY);
 * FROM_PROXY 6 / FROM_HOST 7 (gf_host_classify with GF_NETDEV_F_TRACE_NOTIFY);
 * source = EVENT_SOURCE, hash, len_orig, len_cap, src_label, dst_label, dst_id
 * (u16), reason (the CT result that forwarded it), pad, ifindex — the layout
 * pkg/monitor/datapath_trace.go TraceNotify decodes), followed by the first
 * len_cap bytes of the frame as it was at the call.  Per packet the records are
 * in the order the programs send them (from_netdev / handle_ingress first, the
 * drop record last), packets in batch order.  Call sites: bpf_lxc.c:364,381,
 * 650,669,705,1014, lib/lxc.h:116,168, lib/encap.h:67, bpf_netdev.c:436. */
/* ---- debug notifications (bpf/lib/dbg.h:144-214, DEBUG) ----
 * Programs loaded with GF_LXC_F_DEBUG also append, through
 * gf_policy_ingress_classify(_batches) only, the cilium_dbg* messages of
 * handle_policy (bpf_lxc.c:745-1024, lib/conntrack.h, lib/policy.h, lib/l4.h,
 * lib/lxc.h), one GF_EVENT_RECORD slot each, zero-filled past what the
 * reference writes:
 *   struct debug_msg (20 B: type CILIUM_NOTIFY_DBG_MSG=2, subtype = DBG_*,
 *   source = EVENT_SOURCE = LXC_ID, hash, arg1, arg2, arg3; arg3 = 0 for the
 *   two-argument cilium_dbg) and
 *   struct debug_capture_msg (24 B: type CILIUM_NOTIFY_DBG_CAPTURE=3, subtype =
 *   DBG_CAPTURE_*, source, hash, len_orig, len_cap, arg1, arg2) followed directly
 *   (offset 24) by len_cap frame bytes: zeros here, column batches carry no frames
 * (the layouts pkg/monitor/datapath_debug.go DebugMsg / DebugCapture decode).
 * Per packet, in the order sent: DBG_SKIP_PROXY; DBG_CT_LOOKUP4_1/_2 (6_1/_2);
 * at most one DBG_CT_MATCH (the entry's lifetime as stored when the lookup found
 * it, its rev_nat_index); DBG_CT_VERDICT; with GF_LXC_F_LB_DEBUG also set, the
 * reverse NAT (bpf/lib/lb.h:304-316, 524-538; IPv4: a CT_REPLY packet whose
 * entry has a rev_nat_index and no loopback bit, IPv6: any lookup result whose
 * entry has a rev_nat_index): DBG_LB4/6_REVERSE_NAT_LOOKUP (the index as stored,
 * 0), then on a hit DBG_LB4_REVERSE_NAT (nat->address be32, nat->port be16,
 * lb.h:456) / DBG_LB6_REVERSE_NAT (nat->address.p4, nat->port, lb.h:264), both
 * before a rewrite that may still end in DROP_CSUM_L4, DROP_WRITE_ERROR or
 * reverse_map_l4_port's error; DBG_L4_CREATE; DBG_GENERIC +
 * DBG_L4_POLICY (l4_proxy_lookup); DBG_POLICY_DENIED (also for reply / related
 * packets, which pass anyway); DBG_CT_CREATED4/6 (also before
 * DROP_CT_CREATE_FAILED); in the redirect TRACE_TO_PROXY (if traced), then
 * DBG_CAPTURE_PROXY_POST, DBG_REV_PROXY_UPDATE (IPv4), DBG_TO_HOST (IPv4, not on
 * DROP_PROXYMAP_CREATE_FAILED); then TRACE_TO_LXC or the drop record, last.
 * DROP_INVALID, DROP_UNKNOWN_L3 and DROP_ALL packets send no message at all;
 * DROP_CT_INVALID_HDR and DROP_CT_UNKNOWN_PROTO return before ct_lookup's first
 * message (at most DBG_SKIP_PROXY, which is sent before the lookup).
 * The ring-full rule is the drop records'.  Such a call needs 32 B of device
 * workspace per packet of the batch for the log (kept for later calls); if it
 * cannot be allocated the call returns -ENOMEM. */
#define GF_TRACE_PAYLOAD_LEN 128u   /* TRACE_PAYLOAD_LEN, bpf/lib/common.h:213-215 */
#define GF_EVENT_RECORD 160u
typedef struct gf_event_ring {
    uint8_t  *records;         /* DEVICE, capacity * GF_EVENT_RECORD bytes */
    uint32_t  capacity;        /* records */
    uint32_t *count;           /* DEVICE u32: records appended so far */
} gf_event_ring;
int gf_set_event_ring(const gf_event_ring *ring);   /* NULL disables */

/* ---- per-call statistics (device counter block) ---- */
#define GF_STATS_WORDS 512
/* Adds the counters of the next classify calls into `dev_counters`
 * (GF_STATS_WORDS u64 in DEVICE memory; NULL disables). Layout:
 * [0..255] drop-reason histogram (reason 0 = not dropped), [256..263]
 * action counts, [264..267] CT ret counts, [268] packets, [269] wire bytes,
 * [270] algorithmic bytes touched (per-probe costs of SURVEY.md §8(d)). */
int gf_set_stats_sink(uint64_t *dev_counters);

/* ---- launch profiler (HIP events recorded on the launch stream) ---- */
typedef struct gf_prof_rec {
    char     name[32];     /* kernel / primitive name */
    uint32_t count;        /* launches since gf_prof_enable */
    uint32_t pad;
    double   total_ms;     /* summed event-measured duration */
} gf_prof_rec;
int gf_prof_enable(int on);                       /* clears accumulators */
int gf_prof_read(gf_prof_rec *out, int max);      /* returns records written */

/* ---- device memory helpers for hosts without a GPU runtime binding ---- */
void *gf_dev_alloc(size_t bytes);
int   gf_dev_free(void *p);
int   gf_memcpy_h2d(void *dst, const void *src, size_t bytes, void *stream);
int   gf_memcpy_d2h(void *dst, const void *src, size_t bytes, void *stream);
int   gf_stream_sync(void *stream);
/* Number of visible GPUs; a library built without a device returns 0. */
int   gf_device_count(void);
const char *gf_version(void);
/* sha256 prefix of the sources (cilium_amd/csrc, include/gpuflow.h) this library
 * was compiled from ("unknown" for builds outside __graft_entry__.build()). */
const char *gf_build_id(void);

/* ---- Geneve tunnel mode (--tunnel geneve: bpf/init.sh:287-292 writes ENCAP_GENEVE into
 * node_config.h; GENEVE_OPTS is always in the endpoint header, pkg/endpoint/bpf.go:235-239) ----
 * Receive: a from-overlay program loaded with GF_OVERLAY_F_GENEVE is bpf_overlay.c compiled
 * with ENCAP_GENEVE.  Only handle_ipv6 has the block (bpf_overlay.c:54-67); IPv4 and non-IP
 * frames behave as in VXLAN mode whatever their option columns hold.  For an IPv6 frame, after
 * the length check (len < 54 DROP_INVALID) and before the endpoint lookup:
 *   skb_get_tunnel_opt(skb, buf[64]) < 0 -> DROP_NO_TUNNEL_OPT.  The helper is Linux's
 *     bpf_skb_get_tunnel_opt (net/core/filter.c): -ENOENT when the packet carries no options
 *     (options_len == 0), -ENOMEM when options_len > 64 (the buffer), otherwise options_len
 *     bytes copied into the zero-initialised buffer.
 *   parse_geneve_options (bpf/lib/geneve.h:46-60): DROP_INVALID_GENEVE unless bytes 0-1 are
 *     ff ff (GENEVE_CLASS_EXPERIMENTAL), byte 2 is 1 (GENEVE_TYPE_SECLABEL) and
 *     (byte 3 & 0x1f) == 1 (length << 2 == 4); the three reserved bits are ignored.  Bytes past
 *     options_len are the buffer's zeros, so options_len 1..3 can never be valid.
 * An option failure therefore wins over DROP_NON_LOCAL and over to_host.  The parsed seclabel
 * is not used: the identity handed to ipv6_local_delivery stays tunnel_id.  Both errors end in
 * send_drop_notify_error(skb, ret, TC_ACT_SHOT) like the program's other drops (stage
 * GF_STAGE_OVERLAY, the frame untouched); with GF_OVERLAY_F_TRACE_NOTIFY the
 * TRACE_FROM_OVERLAY record still comes first. */
#define GF_OVERLAY_F_GENEVE (1u << 1)  /* gf_overlay_cfg.flags: ENCAP_GENEVE defined */
#define GF_DROP_NO_TUNNEL_OPT  148     /* DROP_NO_TUNNEL_OPT,  bpf/lib/common.h:242 */
#define GF_DROP_INVALID_GENEVE 149     /* DROP_INVALID_GENEVE, bpf/lib/common.h:243 */
typedef struct gf_tunnel_opts {
    const uint8_t *opt;        /* DEVICE, n * opt_stride; the first bytes of each packet's option area */
    uint32_t       opt_stride; /* 4..64, multiple of 4; opt 4-byte aligned */
    const uint8_t *opt_len;    /* DEVICE, options_len per packet; 0 = no options present */
} gf_tunnel_opts;
/* gf_overlay_classify with the packets' tunnel options.  A program loaded with
 * GF_OVERLAY_F_GENEVE must be called here: through gf_overlay_classify it returns -EINVAL;
 * here -EFAULT for opts == NULL or either column NULL and -EINVAL for a stride outside
 * 4..64, not a multiple of 4, or opt not 4-byte aligned.  A program without the flag ignores
 * opts (NULL included) and is gf_overlay_classify.  Every refusal precedes any launch.  Only
 * the first 4 option bytes of a packet are read (all parse_geneve_options looks at). */
int gf_overlay_classify_opts(int ovl, const gf_overlay_batch *batch, const gf_tunnel_opts *opts,
                             uint32_t now_sec, gf_pipeline_out *out, uint8_t *snap_out, void *stream);
/* Transmit: the tunnel metadata encap_and_redirect (bpf/lib/encap.h:30-81) sets for the
 * from-container packets gf_lxc_egress_classify reports with GF_EG_F_ENCAP, besides
 * gf_egress_out.tunnel_ip (bpf_tunnel_key.remote_ipv4).  lxc_id: the batch's column; records:
 * the call's output; all pointers DEVICE.  For a record with GF_EG_F_ENCAP:
 *   tunnel_id[i] = bpf_tunnel_key.tunnel_id = SECLABEL of the program in slot lxc_id[i];
 *   opt[8 i .. 8 i + 8] = GENEVE_OPTS: ff ff 01 01 and the identity as a big-endian u32
 *     (writeGeneve, pkg/endpoint/bpf.go:375-394; ReadOpts emits len >> 2, pkg/geneve/geneve.go:69;
 *     bpf/lxc_config.h:35 shows the shape); opt_len[i] = 8.
 * Every other record (an empty slot included): zeros.  Neither helper can fail on this path, so
 * DROP_WRITE_ERROR is unreachable and no record changes.  bpf_netdev and FROM_HOST pass an
 * empty buffer (sz 0) and are not part of this call.  The columns have the layout
 * gf_overlay_batch.tunnel_id and gf_tunnel_opts (opt_stride 8) take on the receiving node.
 * -EBADF (not a cilium_policy array), -EFAULT (a NULL pointer), -EINVAL (opt not 4-byte
 * aligned), -E2BIG; n == 0 returns 0. */
int gf_lxc_egress_tunnel_meta(int policy_array, const uint16_t *lxc_id, const gf_egress_out *records, uint32_t n,
                              uint32_t *tunnel_id, uint8_t *opt /* n*8 */, uint8_t *opt_len, void *stream);

/* ---- VXLAN / Geneve on the wire: gf_tunnel_encap, gf_tunnel_decap ----
 * The step the reference leaves to the kernel's cilium_vxlan / cilium_geneve device
 * (bpf/init.sh:295-300, "type $MODE external"): redirect(ENCAP_IFINDEX) sends into it and
 * from-overlay receives from it.  The reference holds no encapsulation code; it only defines the
 * metadata (bpf/lib/encap.h:30-81).  The headers follow their RFCs: IPv4 RFC 791, UDP RFC 768,
 * VXLAN RFC 7348 section 5, Geneve RFC 8926 section 3.4.  The underlay is IPv4 only
 * (bpf_tunnel_key carries remote_ipv4 only).  Outer frame:
 *   Ethernet 14 | IPv4 20 (IHL 5 on transmit) | UDP 8 | tunnel header 8 | Geneve options | inner frame
 *   VXLAN:  08 00 00 00 | VNI(3) | 00          Geneve: opt_len/4 | 00 | 65 58 | VNI(3) | 00
 * VNI = tunnel_id & 0xffffff.  What the kernel's device would choose itself is configuration here
 * (INTEGRATION.md lists what an agent would pass).  Every IPv4 address of these calls (local_ip,
 * remote_ip, outer_saddr) has the form of gf_egress_out.tunnel_ip: 10.0.0.1 is 0x0a000001, sent
 * most significant byte first.  These are this library's rules; a Linux device differs in places
 * (DESIGN.md). */
#define GF_TUN_VXLAN  0
#define GF_TUN_GENEVE 1
#define GF_TUN_F_UDP_CSUM (1u << 0)   /* transmit: compute the outer UDP checksum (else 0) */
#define GF_TUN_F_DF       (1u << 1)   /* transmit: set DF in the outer IPv4 header */
typedef struct gf_tunnel_cfg {
    uint32_t mode;          /* GF_TUN_VXLAN | GF_TUN_GENEVE */
    uint32_t flags;         /* GF_TUN_F_* */
    uint32_t local_ip;      /* outer saddr on transmit; on receive the daddr a tunnel packet must have (0 = any) */
    uint16_t dst_port;      /* host order: 8472 or 4789 for VXLAN, 6081 for Geneve; never defaulted (0: -EINVAL) */
    uint16_t sport_min, sport_max;  /* source port = sport_min + ((u64)flow_hash * (sport_max - sport_min) >> 32) */
    uint8_t  ttl, tos;
    uint8_t  src_mac[6], dst_mac[6];   /* outer Ethernet; dst_mac is the next hop unless the batch has a column */
} gf_tunnel_cfg;            /* 32 B */
/* -EFAULT (NULL), -EINVAL (mode, unknown flags, dst_port 0, sport_min > sport_max). */
int gf_tunnel_load(const gf_tunnel_cfg *cfg);

#define GF_TUN_ST_OK            0
#define GF_TUN_ST_SKIPPED       1   /* encap: select[i] == 0 */
#define GF_TUN_ST_SHORT         2   /* encap: len < 14 */
#define GF_TUN_ST_BAD_OPT       3   /* encap, Geneve: opt_len not a multiple of 4, > opt_stride or > 64 */
#define GF_TUN_ST_TRUNCATED     4   /* encap with GF_TUN_F_UDP_CSUM: len > snap_stride, the datagram cannot be summed */
#define GF_TUN_ST_NOT_TUNNEL    5   /* decap: not addressed to this tunnel endpoint */
#define GF_TUN_ST_BAD_OUTER     6   /* decap: malformed Ethernet / IPv4 / UDP */
#define GF_TUN_ST_BAD_HDR       7   /* decap: malformed VXLAN / Geneve header */
#define GF_TUN_ST_BAD_CSUM      8   /* decap: the UDP checksum was verified and is wrong */
#define GF_TUN_ST_OK_UNVERIFIED 9   /* decap: a UDP checksum is present but the datagram is longer than the snap */

typedef struct gf_tunnel_tx {
    gf_frames frames;            /* DEVICE inner frames, snap_stride 14..256 as everywhere else */
    const uint32_t *remote_ip;   /* DEVICE, as gf_egress_out.tunnel_ip; required */
    const uint32_t *tunnel_id;   /* DEVICE, required */
    const uint8_t  *opt; uint32_t opt_stride; const uint8_t *opt_len;   /* Geneve only, gf_tunnel_opts' rules; opt NULL = no options */
    const uint8_t  *select;      /* DEVICE, may be NULL: 0 = leave this frame out */
    const uint32_t *flow_hash;   /* DEVICE, may be NULL (source port sport_min) */
    const uint16_t *ip_id;       /* DEVICE, may be NULL (identification 0) */
    const uint8_t  *dst_mac;     /* DEVICE n*6, may be NULL (gf_tunnel_cfg.dst_mac) */
} gf_tunnel_tx;                  /* 96 B */
/* Per frame, first match: SKIPPED, SHORT, BAD_OPT, TRUNCATED, else OK.  For an OK frame
 * out_len[i] = len + 50 (+ opt_len in Geneve mode), the outer total length and UDP length come from
 * the true len, and row i of out (out_stride bytes per frame) holds the outer headers followed by
 * the first min(len, snap_stride) inner bytes, cut at out_stride; no byte of the row past those is
 * written.  The IPv4 header checksum is always set.  The UDP checksum is 0 without
 * GF_TUN_F_UDP_CSUM; with it, it covers the pseudo-header and the whole datagram, a computed 0 is
 * sent as 0xffff, and a frame with len > snap_stride is TRUNCATED.  Every other status: out_len[i]
 * = 0 and the row untouched.  len + 36 + opt_len must fit the 16-bit total length (no GSO, no
 * fragmentation).  A VXLAN-mode handle ignores the option columns.
 * -EBADF; -EFAULT (a NULL batch, frame pointer, remote_ip, tunnel_id, out, out_len or status, or
 * opt without opt_len); -EINVAL (snap_stride outside 14..256; out_stride not a multiple of 16,
 * < 128 or > 512; out not 16-byte aligned or == frames.snap; Geneve opt_stride outside 4..64, not a
 * multiple of 4, or opt not 4-byte aligned); -E2BIG; n == 0 returns 0.  Every refusal precedes any
 * launch. */
int gf_tunnel_encap(int tun, const gf_tunnel_tx *b, uint8_t *out, uint32_t out_stride,
                    uint32_t *out_len, uint8_t *status, void *stream);
/* The select column of gf_tunnel_encap from the records of a classify call (rec_kind as
 * gf_respond_calls): GF_REC_EGRESS: eg_flags & GF_EG_F_ENCAP; GF_REC_PIPELINE: action REDIRECT and
 * ifindex_lo == gf_node_cfg.encap_ifindex != 0 (gf_pipeline_classify_tunnel, gf_host_classify).
 * -EINVAL (rec_kind), -EFAULT, -E2BIG; n == 0 returns 0. */
int gf_tunnel_select(const void *records, uint32_t rec_kind, uint32_t n, uint8_t *select, void *stream);

typedef struct gf_tunnel_rx_out {
    uint8_t  *inner; uint32_t inner_stride;  /* 14..256 */
    uint32_t *inner_len, *tunnel_id, *outer_saddr;
    uint8_t  *opt; uint32_t opt_stride; uint8_t *opt_len;    /* gf_tunnel_opts' layout; may be NULL in VXLAN mode */
    uint8_t  *status;
} gf_tunnel_rx_out;              /* 72 B */
/* outer: DEVICE frames as received from the wire, snap_stride 64..512.  The output columns have
 * the layout gf_overlay_batch and gf_tunnel_opts take, so they go to gf_overlay_classify_opts
 * without a copy.  cap = min(len, snap_stride).  Status per frame, first match:
 *   cap < 14                                                             BAD_OUTER
 *   ethertype != 0x0800                                                  NOT_TUNNEL
 *   cap < 34                                                             BAD_OUTER
 *   protocol != 17, MF set or fragment offset != 0, or daddr != local_ip (when set)  NOT_TUNNEL
 *   version != 4 or IHL < 5; the UDP header not inside cap               BAD_OUTER
 *   destination port != dst_port                                         NOT_TUNNEL
 *   IPv4 total length != len - 14 or UDP length != len - 14 - 4 IHL; the tunnel header not
 *     inside cap; the IPv4 header checksum wrong (IHL > 5 is accepted and skipped)  BAD_OUTER
 *   VXLAN: flags byte != 0x08 or a reserved byte != 0.  Geneve: version != 0, protocol != 0x6558,
 *     the C bit set, or the options run past the datagram or the snap    BAD_HDR
 *   UDP checksum != 0 and len <= snap_stride: wrong sum BAD_CSUM; len > snap_stride OK_UNVERIFIED
 *   else OK.
 * OK and OK_UNVERIFIED: inner_len = len - headers, row i of inner holds the first
 * min(inner_len, cap - headers, inner_stride) inner bytes (nothing past them is written),
 * tunnel_id = VNI, outer_saddr, opt_len = the option bytes present (0 in VXLAN mode) and, in
 * Geneve mode, the first min(opt_len, opt_stride) option bytes in row i of opt.  Every other status:
 * inner_len = 0 and nothing else written.
 * -EBADF; -EFAULT (NULL outer, out, a frame pointer, inner, inner_len, tunnel_id, outer_saddr or
 * status; opt or opt_len in Geneve mode); -EINVAL (snap_stride outside 64..512, inner_stride
 * outside 14..256, Geneve opt_stride outside 4..64 or not a multiple of 4, opt not 4-byte aligned,
 * inner == outer->snap); -E2BIG; n == 0 returns 0. */
int gf_tunnel_decap(int tun, const gf_frames *outer, const gf_tunnel_rx_out *out, void *stream);

/* ---- draining the event ring on the device: gf_event_filter_load, gf_event_drain ----
 * The consumer's half of the monitor path: `cilium monitor --type --from --to --related-to`
 * (cilium/cmd/monitor.go:108-156) applied to a ring of GF_EVENT_RECORD slots before anything
 * crosses PCIe.  match() (monitor.go:144-156) gets, per record (monitor.go:165,182,199,215):
 *   type   byte 0 (1 drop, 2 debug, 3 capture, 4 trace: pkg/monitor/types.go:29-33)
 *   src    the u16 at byte 2 (Source of all four layouts)
 *   dst    drop: uint16(dn.DstID), the low 16 bits of the u32 at byte 24 (0x10005 matches --to 5);
 *          trace: the u16 at byte 24; debug and capture: 0
 * and passes the record when, in this order: type_mask is 0 or has bit `type`; from is not given
 * or holds src; to is not given or holds dst; related is not given or holds src or dst.  A record
 * whose type is not 1..4 ("Unknown event" in the reference, whatever the filter) never passes and
 * is counted in `unknown`. */
#define GF_EVF_MAX_IDS 65536u
typedef struct gf_event_filter_cfg {
    uint32_t type_mask;        /* bit t set = message type t passes; 0 = no --type given, every type passes */
    const uint16_t *from;  uint32_t n_from;      /* HOST lists; n == 0 = flag not given */
    const uint16_t *to;    uint32_t n_to;
    const uint16_t *related; uint32_t n_related;
} gf_event_filter_cfg;         /* 56 B */
/* A filter handle (gf_obj_close frees it); the lists are copied.  On the device the filter is three
 * 65536-bit bitmaps, built here and uploaded by the handle's first gf_event_drain (the one call that
 * waits for a copy).  -EFAULT (NULL cfg, a NULL list with n != 0), -EINVAL (a type_mask bit outside
 * 1..4), -E2BIG (a list longer than GF_EVF_MAX_IDS). */
int gf_event_filter_load(const gf_event_filter_cfg *cfg);

#define GF_EVD_F_PACKED (1u << 0)   /* wire-length records instead of 160-B slots */
#define GF_EVD_F_RESET  (1u << 1)   /* set *ring->count = 0 once the drain has read it */
#define GF_EVD_MAX_WINDOW (1u << 24)
typedef struct gf_event_drain_out {  /* DEVICE, written by the call */
    uint32_t count;        /* *ring->count as the call found it */
    uint32_t lost;         /* max(count, capacity) - capacity: the ring's overrun */
    uint32_t seen;         /* records examined: those of [first, min(count, capacity, first + max_n)) */
    uint32_t matched;      /* of those, records that pass the filter */
    uint32_t written;      /* of those, records stored in out (a prefix, in ring order) */
    uint32_t unknown;      /* records whose type is not 1..4: never matched */
    uint64_t bytes;        /* bytes stored in out */
    uint32_t by_type[5];   /* matched records per type (index 0 unused) */
    uint32_t pad;
} gf_event_drain_out;      /* 56 B */
/* Examines the records [first, min(*ring->count, capacity, first + max_n)) of `ring` (max_n == 0:
 * to the end, at most GF_EVD_MAX_WINDOW records) and stores those that pass `filter` in `out`, in
 * ring order.  Without GF_EVD_F_PACKED each stored record is its whole 160-byte slot and written =
 * min(matched, out_bytes / 160).  With it a record takes its wire length (drop and trace 32 +
 * len_cap, debug message 20, capture 24 + len_cap; len_cap is the u32 at byte 12; the result
 * clamped to 160) rounded up to a multiple of 8 with zero bytes, and records are stored while the
 * running total fits out_bytes: the first one that does not fit ends the output.  out_off (may be
 * NULL; room for min(max_n ? max_n : GF_EVD_MAX_WINDOW, capacity) + 1 u32) receives the byte offset
 * of every stored record and the total at index `written`.  No byte of out past res->bytes and no
 * word of out_off past index `written` is written.  res is always written; first >= min(count,
 * capacity) gives seen = 0.  out_bytes == 0 (out may then be NULL) only counts.
 * The call is stream-ordered like the classify calls that fill the ring (with the ring of
 * gf_set_event_ring it also takes its turn among calls on other streams): it reads *ring->count on
 * the device and waits for nothing on the host; with GF_EVD_F_RESET the ring is empty for the next
 * classify call on that stream.  Three launches (k_evd_count, k_evd_scan, k_evd_scatter); no block
 * waits for another.  16-byte copies when records and out are 16-byte aligned (slot mode), 8-byte
 * copies when both are 8-byte aligned (packed mode), byte copies otherwise.
 * Every refusal precedes any launch and writes nothing: -EBADF (filter); -EFAULT (NULL ring,
 * ring->records, ring->count or res; NULL out with out_bytes != 0); -EINVAL (an unknown flag, out
 * overlapping the ring's records, records not 4-byte aligned); -E2BIG (max_n > GF_EVD_MAX_WINDOW). */
int gf_event_drain(int filter, const gf_event_ring *ring, uint32_t first, uint32_t max_n, uint32_t flags,
                   uint8_t *out, uint64_t out_bytes, uint32_t *out_off, gf_event_drain_out *res, void *stream);

/* ---- forwarding the verdicts: gf_forward_load, gf_forward_queues, gf_forward_frames ----
 * The last step of a chain of frame operators.  In the reference a verdict moves the packet:
 * TC_ACT_SHOT frees the skb, TC_ACT_OK hands it to the stack, redirect(ifindex) puts it on that
 * device's queue.  Here: a stable multi-way partition of the classified frames into at most
 * GF_FWD_MAX_QUEUES output queues, in two calls, so that the partition works for any queue column
 * and not only for the record kinds below.
 *
 * gf_forward_queues: queue[i] from record i of a classify call, the first row that matches:
 *   1  GF_REC_PIPELINE with stage == GF_STAGE_XDP (the action byte is XDP_DROP)   GF_FWD_DROP
 *   2  a responder tail call is pending (gf_respond_calls yields a call other than
 *      GF_CALL_NONE; no frame byte is read for this):
 *        GF_REC_EGRESS    eg_flags & (GF_EG_F_ARP | GF_EG_F_RESPONDER | GF_EG_F_ICMP6_TE)
 *        GF_REC_PIPELINE  flags & (GF_PIPE_F_ICMP6_TE | GF_PIPE_F_RESPONDER)         responder_queue
 *   3  action TC_ACT_SHOT                                                         GF_FWD_DROP
 *   4  action TC_ACT_OK                                                           stack_queue
 *   5  action TC_ACT_REDIRECT: the queue of the entry for the record's ifindex_lo, or
 *      default_queue without one; GF_REC_LB, whose record carries no ifindex (bpf_lb has one
 *      target, LB_REDIRECT): always default_queue
 *   6  any other action byte                                                      GF_FWD_DROP
 * GF_REC_LB records have no stage and no flags: rows 3 to 6 only. */
#define GF_FWD_MAX_QUEUES 64
#define GF_FWD_DROP       0xffu      /* queue value: the frame is not forwarded */
#define GF_REC_LB         3          /* gf_lb_out (12 B), next to GF_REC_EGRESS / GF_REC_PIPELINE */
typedef struct gf_forward_ifindex { uint16_t ifindex_lo; uint8_t queue; uint8_t pad; } gf_forward_ifindex;
typedef struct gf_forward_cfg {
    uint32_t n_queues;          /* 1..GF_FWD_MAX_QUEUES */
    uint8_t  stack_queue;       /* TC_ACT_OK frames; a queue < n_queues or GF_FWD_DROP */
    uint8_t  responder_queue;   /* frames with a responder tail call pending (for gf_respond) */
    uint8_t  default_queue;     /* REDIRECT to an ifindex without an entry; every REDIRECT of GF_REC_LB */
    uint8_t  pad;
    uint32_t n_ifindex;
    const gf_forward_ifindex *ifindex;   /* HOST; a later entry for the same ifindex_lo wins */
} gf_forward_cfg;
/* A forward handle (gf_obj_close frees it); the entries are copied.  On the device the rule is a
 * 65536-byte ifindex_lo -> queue table (default_queue where there is no entry), built here and
 * uploaded by the handle's first gf_forward_queues (the one call that waits for a copy).
 * -EFAULT (NULL cfg; n_ifindex > 0 with a NULL ifindex), -EINVAL (n_queues outside
 * 1..GF_FWD_MAX_QUEUES; stack_queue, responder_queue, default_queue or an entry's queue that is
 * neither < n_queues nor GF_FWD_DROP). */
int gf_forward_load(const gf_forward_cfg *cfg);
/* queue[i] (DEVICE, n bytes) from the records (DEVICE) of a classify call, by the table above.
 * One launch (k_fwd_queues).  -EBADF (not a forward handle), -EFAULT (n > 0 with NULL records or
 * queue), -EINVAL (rec_kind), -E2BIG (n > 2^30); n == 0 returns 0. */
int gf_forward_queues(int fwd, const void *records, uint32_t rec_kind, uint32_t n, uint8_t *queue, void *stream);

/* Row i of `frames` is forwarded iff queue[i] < n_queues; GF_FWD_DROP and every other byte
 * >= n_queues are not (the latter are counted in counts[3]).  The forwarded rows are packed
 * queue-major, in arrival order inside a queue (the partition is stable): queue q owns the output
 * rows [qoff[q], qoff[q + 1]).  A packed row is the whole input row (snap_stride bytes, verbatim,
 * the bytes past len included); len[r] is its wire length and index[r] its batch index i, the
 * handle for the record and any side column the caller carries along.  qoff and counts[0] come
 * from the full counts whatever max_out is; output row r is written iff r < max_out, and nothing
 * at or past row counts[2] is written in snap, len or index: the call is asynchronous and cannot
 * fail late.  There is no in-place mode.  The call takes no handle and no map locks, and touches
 * neither the event ring nor the stats sink.  Three launches after the queue column (k_fwd_count,
 * k_fwd_scan, k_fwd_scatter); no block waits for another.  Rows move in 16-byte pieces when
 * frames->snap, out->snap and snap_stride are multiples of 16, in 4-byte pieces when of 4, else
 * byte by byte.
 * Errors, all before anything is launched or written: -EFAULT (NULL frames, queue, out, qoff or
 * counts; n > 0 with a NULL frames->snap or frames->len; out->snap without out->len), -EINVAL
 * (n_queues outside 1..GF_FWD_MAX_QUEUES; n > 0 with snap_stride outside 14..256; out->snap NULL
 * with out->len or out->index; an output buffer that overlaps frames->snap, frames->len or queue),
 * -E2BIG (n > 2^30).  n == 0 returns 0 and writes qoff and counts (zeros). */
typedef struct gf_forward_out {
    uint8_t  *snap;     /* DEVICE, max_out * snap_stride: whole rows, queue-major, arrival order inside a queue; may be NULL */
    uint32_t *len;      /* DEVICE, max_out; NULL only with snap NULL */
    uint32_t *index;    /* DEVICE, max_out: batch index of each packed row; may be NULL */
    uint32_t  max_out;
    uint32_t *qoff;     /* DEVICE, n_queues + 1 words, required: queue q owns rows [qoff[q], qoff[q+1]) */
    uint32_t *counts;   /* DEVICE, 4 words, required: [0] forwarded = qoff[n_queues], [1] not forwarded,
                           [2] rows written = min([0], max_out) (0 with snap NULL), [3] queue bytes >= n_queues other than GF_FWD_DROP */
} gf_forward_out;
int gf_forward_frames(const gf_frames *frames, const uint8_t *queue, uint32_t n_queues,
                      const gf_forward_out *out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* GPUFLOW_H */
