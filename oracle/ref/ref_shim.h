/*
 * ref_shim.h — host implementations of the BPF helpers that api.h declares
 * (through the BPF_FUNC override of the wrapper unit) for one reference
 * program compiled as ordinary host code.  TEST INFRASTRUCTURE ONLY.
 *
 * Included LAST in a wrapper unit, after the reference program: the api.h
 * prototypes are static, so the definitions must sit in the same unit.  The
 * generated config headers (oracle/refdiff.py) provide
 *   REF_MAPS      X(map object, "scenario map name") for every bound map
 *   REF_ENTRY     the program's entry function
 *   REF_XDP       defined when the entry takes a struct xdp_md
 * Helper semantics follow the kernel's documented behaviour (bpf-helpers(7),
 * net/core/filter.c): offset > 0xffff or a range past skb->len is -EFAULT,
 * unknown flag bits are -EINVAL.  The checksum arithmetic lives in the runner
 * (ref_runner.c, from RFC 1071 / RFC 1624).  Every helper that the compared
 * programs are not expected to reach sets the packet's "unmodelled" flag.
 */
#ifndef GF_REF_SHIM_H
#define GF_REF_SHIM_H
#include <errno.h>
#include <setjmp.h>
#include "ref_rt.h"

static struct ref_rt *ref_RT;
static struct ref_pkt *ref_PKT;
static jmp_buf ref_jmp;
static int ref_tail_ret;

#define REF_UNMODELLED() (ref_RT->cur.unmodelled = 1)

static void *map_lookup_elem(void *map, const void *key) { return ref_RT->map_lookup(ref_RT, map, key); }
static int map_update_elem(void *map, const void *key, const void *value, uint32_t flags)
{
	return ref_RT->map_update(ref_RT, map, key, value, flags);
}
static int map_delete_elem(void *map, const void *key) { return ref_RT->map_delete(ref_RT, map, key); }
static uint64_t ktime_get_ns(void) { return ref_RT->ktime_get_ns(ref_RT); }
static uint32_t get_prandom_u32(void) { return ref_RT->prandom(ref_RT); }

#ifndef REF_XDP
static uint32_t get_hash_recalc(struct __sk_buff *skb) { return skb->hash = ref_PKT->hash; }

static int ref_range(struct __sk_buff *skb, uint32_t off, uint32_t len)
{
	if (off > 0xffff || (uint64_t)off + len > skb->len)
		return -EFAULT;
	return 0;
}

static int skb_load_bytes(struct __sk_buff *skb, uint32_t off, void *to, uint32_t len)
{
	if (ref_range(skb, off, len) < 0) {
		memset(to, 0, len);
		return -EFAULT;
	}
	memcpy(to, ref_PKT->data + off, len);
	return 0;
}

static int skb_store_bytes(struct __sk_buff *skb, uint32_t off, const void *from, uint32_t len, uint32_t flags)
{
	if (flags & ~(BPF_F_RECOMPUTE_CSUM | BPF_F_INVALIDATE_HASH))
		return -EINVAL;
	if (ref_range(skb, off, len) < 0)
		return -EFAULT;
	__builtin_memmove(ref_PKT->data + off, from, len);
	if (flags & BPF_F_INVALIDATE_HASH)
		skb->hash = 0;
	return 0;
}

static int l3_csum_replace(struct __sk_buff *skb, uint32_t off, uint32_t from, uint32_t to, uint32_t flags)
{
	return ref_RT->l3_csum_replace(ref_PKT->data, skb->len, off, from, to, flags);
}

static int l4_csum_replace(struct __sk_buff *skb, uint32_t off, uint32_t from, uint32_t to, uint32_t flags)
{
	return ref_RT->l4_csum_replace(ref_PKT->data, skb->len, off, from, to, flags);
}

static int redirect(int ifindex, uint32_t flags)
{
	if (flags & ~BPF_F_INGRESS)
		return TC_ACT_SHOT;
	ref_RT->cur.redirect_called = 1;
	ref_RT->cur.redirect_ifindex = (uint32_t)ifindex;
	ref_RT->cur.redirect_flags = flags;
	return TC_ACT_REDIRECT;
}

/* bpf_perf_event_output on an skb: the upper flag bits carry the number of packet bytes to append */
static int ref_event_output(struct __sk_buff *skb, void *map, uint64_t index, const void *data, uint32_t size)
{
	uint64_t cap = (index & BPF_F_CTXLEN_MASK) >> 32;

	(void)map;
	if ((index & ~(BPF_F_CTXLEN_MASK | BPF_F_INDEX_MASK)) || cap > skb->len)
		return -EFAULT;
	ref_RT->event(ref_RT, data, size, ref_PKT->data, (uint32_t)cap);
	return 0;
}

/* A tail call that succeeds never returns.  Targets inside the unit run here and their
 * return value becomes the program's; any other (map, index) pair is recorded and the
 * program counts as left. */
static void tail_call(struct __sk_buff *skb, void *map, uint32_t index)
{
#if !defined SKIP_CALLS_MAP && defined DROP_NOTIFY
	if (map == (void *)&CALLS_MAP && index == CILIUM_CALL_DROP_NOTIFY) {
		ref_tail_ret = __send_drop_notify(skb);
		longjmp(ref_jmp, 1);
	}
#endif
	(void)skb;
	ref_RT->cur.tail_called = 1;
	ref_RT->cur.tail_map = ref_RT->bind_index(ref_RT, map);
	ref_RT->cur.tail_index = index;
	longjmp(ref_jmp, 2);
}
#else /* REF_XDP */
static uint32_t get_hash_recalc(struct __sk_buff *skb) { (void)skb; REF_UNMODELLED(); return 0; }
static int skb_load_bytes(struct __sk_buff *skb, uint32_t off, void *to, uint32_t len)
{
	(void)skb; (void)off; memset(to, 0, len); REF_UNMODELLED(); return -EFAULT;
}
static int skb_store_bytes(struct __sk_buff *skb, uint32_t off, const void *from, uint32_t len, uint32_t flags)
{
	(void)skb; (void)off; (void)from; (void)len; (void)flags; REF_UNMODELLED(); return -EFAULT;
}
static int l3_csum_replace(struct __sk_buff *skb, uint32_t off, uint32_t from, uint32_t to, uint32_t flags)
{
	(void)skb; (void)off; (void)from; (void)to; (void)flags; REF_UNMODELLED(); return -EFAULT;
}
static int l4_csum_replace(struct __sk_buff *skb, uint32_t off, uint32_t from, uint32_t to, uint32_t flags)
{
	(void)skb; (void)off; (void)from; (void)to; (void)flags; REF_UNMODELLED(); return -EFAULT;
}
static int redirect(int ifindex, uint32_t flags) { (void)ifindex; (void)flags; REF_UNMODELLED(); return TC_ACT_SHOT; }
static int ref_event_output(struct __sk_buff *skb, void *map, uint64_t index, const void *data, uint32_t size)
{
	(void)skb; (void)map; (void)index; (void)data; (void)size; REF_UNMODELLED(); return -EFAULT;
}
static void tail_call(struct __sk_buff *skb, void *map, uint32_t index)
{
	(void)skb; (void)map; (void)index; REF_UNMODELLED();
}
#endif

static int csum_diff(void *from, uint32_t from_size, void *to, uint32_t to_size, uint32_t seed)
{
	return ref_RT->csum_diff(from, from_size, to, to_size, seed);
}

/* ---- everything else: unmodelled ---- */
static void trace_printk(const char *fmt, int fmt_size, ...) { (void)fmt; (void)fmt_size; REF_UNMODELLED(); }
static uint32_t get_smp_processor_id(void) { REF_UNMODELLED(); return 0; }
static uint32_t get_cgroup_classid(struct __sk_buff *skb) { (void)skb; REF_UNMODELLED(); return 0; }
static uint32_t get_route_realm(struct __sk_buff *skb) { (void)skb; REF_UNMODELLED(); return 0; }
static uint32_t set_hash_invalid(struct __sk_buff *skb) { (void)skb; REF_UNMODELLED(); return 0; }
static int skb_under_cgroup(void *map, uint32_t index) { (void)map; (void)index; REF_UNMODELLED(); return -EINVAL; }
static int clone_redirect(struct __sk_buff *skb, int ifindex, uint32_t flags)
{
	(void)skb; (void)ifindex; (void)flags; REF_UNMODELLED(); return -EINVAL;
}
static int skb_change_type(struct __sk_buff *skb, uint32_t type) { (void)skb; (void)type; REF_UNMODELLED(); return -EINVAL; }
static int skb_change_proto(struct __sk_buff *skb, uint32_t proto, uint32_t flags)
{
	(void)skb; (void)proto; (void)flags; REF_UNMODELLED(); return -EINVAL;
}
static int skb_change_tail(struct __sk_buff *skb, uint32_t nlen, uint32_t flags)
{
	(void)skb; (void)nlen; (void)flags; REF_UNMODELLED(); return -EINVAL;
}
static int skb_vlan_push(struct __sk_buff *skb, uint16_t proto, uint16_t vlan_tci)
{
	(void)skb; (void)proto; (void)vlan_tci; REF_UNMODELLED(); return -EINVAL;
}
static int skb_vlan_pop(struct __sk_buff *skb) { (void)skb; REF_UNMODELLED(); return -EINVAL; }
static int skb_get_tunnel_key(struct __sk_buff *skb, struct bpf_tunnel_key *to, uint32_t size, uint32_t flags)
{
	(void)skb; (void)flags; memset(to, 0, size); REF_UNMODELLED(); return -EINVAL;
}
static int skb_set_tunnel_key(struct __sk_buff *skb, const struct bpf_tunnel_key *from, uint32_t size, uint32_t flags)
{
	(void)skb; (void)from; (void)size; (void)flags; REF_UNMODELLED(); return -EINVAL;
}
static int skb_get_tunnel_opt(struct __sk_buff *skb, void *to, uint32_t size)
{
	(void)skb; memset(to, 0, size); REF_UNMODELLED(); return -EINVAL;
}
static int skb_set_tunnel_opt(struct __sk_buff *skb, const void *from, uint32_t size)
{
	(void)skb; (void)from; (void)size; REF_UNMODELLED(); return -EINVAL;
}

/* the LLVM BPF load intrinsics that api.h declares: no host counterpart */
unsigned long long load_byte(void *skb, unsigned long long off) { (void)skb; (void)off; REF_UNMODELLED(); return 0; }
unsigned long long load_half(void *skb, unsigned long long off) { (void)skb; (void)off; REF_UNMODELLED(); return 0; }
unsigned long long load_word(void *skb, unsigned long long off) { (void)skb; (void)off; REF_UNMODELLED(); return 0; }

/* ---- what the runner calls ---- */
struct ref_bind_row { const void *map; const char *name; };
#define X(OBJ, NAME) { &OBJ, NAME },
static const struct ref_bind_row ref_binds[] = { REF_MAPS { 0, 0 } };
#undef X

__attribute__((visibility("default"))) void ref_bind(struct ref_rt *rt)
{
	ref_RT = rt;
	skb_event_output = ref_event_output;        /* BPF_FUNC2 leaves this one a pointer */
	for (const struct ref_bind_row *r = ref_binds; r->map; r++)
		rt->bind(rt, r->map, r->name);
}

__attribute__((visibility("default"))) void ref_run(struct ref_rt *rt, struct ref_pkt *p)
{
	int how;

	ref_RT = rt;
	ref_PKT = p;
#ifndef REF_XDP
	static struct __sk_buff skb;                /* static: read again after a longjmp */

	memset(&skb, 0, sizeof(skb));
	skb.len = p->len;
	skb.protocol = p->protocol;
	skb.mark = p->mark;
	skb.ifindex = p->ifindex;
	skb.ingress_ifindex = p->ingress_ifindex;
	skb.tc_index = p->tc_index;
	skb.hash = p->hash;
	memcpy(skb.cb, p->cb, sizeof(skb.cb));
	skb.data = (uint32_t)(uintptr_t)p->data;
	skb.data_end = skb.data + p->len;
	how = setjmp(ref_jmp);
	if (how == 0)
		rt->cur.ret = REF_ENTRY(&skb);
	else if (how == 1)
		rt->cur.ret = ref_tail_ret;
	else
		rt->cur.ret = INT32_MIN;               /* left through a recorded tail call */
	memcpy(rt->cur.cb, skb.cb, sizeof(skb.cb));
#else
	struct xdp_md xdp;

	(void)how;
	xdp.data = (uint32_t)(uintptr_t)p->data;
	xdp.data_end = xdp.data + p->len;
	rt->cur.ret = REF_ENTRY(&xdp);
#endif
}

#endif
