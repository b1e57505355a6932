// gf_host_ctx.h — the host side begins: what every entry point stands on (included by
// gf_kernels.hip after the last device stage; it leans on gf_internal.h's host objects only).
//
//   Prof, ProfScope, HostMarks   the launch profiler
//   Workspace, CallCtx, CtxScope one context per stream: the device workspaces of a call
//   check_cols                   the column checks the classify calls share
//   CallOrder                    device-side order of the calls that share an object

// ================================================================ host: programs
namespace {

// ---- launch profiler: HIP events on the launch stream around each kernel ----
struct ProfEntry { std::string name; hipEvent_t a, b; };
struct Prof {
    bool on = false;
    std::mutex mu;                     // concurrent classify calls record launches
    std::vector<ProfEntry> pending;
    std::map<std::string, std::pair<uint32_t, double>> acc;
};
Prof &prof() { static Prof p; return p; }
struct ProfScope {
    ProfEntry e{};
    bool on;
    hipStream_t s;
    ProfScope(const char *n, hipStream_t s_) : on(prof().on), s(s_) {
        if (!on) return;
        e.name = n;
        // timing only: no system-scope fence (an L2 writeback) at each launch boundary
        (void)hipEventCreateWithFlags(&e.a, hipEventDisableSystemFence);
        (void)hipEventCreateWithFlags(&e.b, hipEventDisableSystemFence);
        (void)hipEventRecord(e.a, s);
    }
    ~ProfScope() {
        if (!on) return;
        (void)hipEventRecord(e.b, s);
        std::lock_guard<std::mutex> g(prof().mu);
        prof().pending.push_back(e);
    }
};
void prof_drain() {
    std::lock_guard<std::mutex> g(prof().mu);
    for (auto &e : prof().pending) {
        float ms = 0;
        if (hipEventSynchronize(e.b) == hipSuccess && hipEventElapsedTime(&ms, e.a, e.b) == hipSuccess) {
            auto &a = prof().acc[e.name];
            a.first++;
            a.second += ms;
        }
        (void)hipEventDestroy(e.a);
        (void)hipEventDestroy(e.b);
    }
    prof().pending.clear();
}

struct Workspace {
    DevBuf rec, keys, skeys, perm, tcnt, off, tmp, sched, order;
    DevBuf sb, st0, st1;               // single-packet buckets in index order (the egress passes)
};
// GF_HOST_PROF (diagnosis): the host time of a classify call's phases, one line
// per call on stderr (where a call waits on the device, or spends its launches).
struct HostMarks {
    using clk = std::chrono::steady_clock;
    bool on;
    clk::time_point t0, last;
    char buf[768];
    int len = 0;
    HostMarks *prev;
    static HostMarks *&cur() { static thread_local HostMarks *c = nullptr; return c; }
    HostMarks() : on(getenv("GF_HOST_PROF") != nullptr), prev(cur()) {
        buf[0] = 0;
        if (on) { t0 = last = clk::now(); cur() = this; }
    }
    static double us(clk::duration d) { return std::chrono::duration<double, std::micro>(d).count(); }
    void mark(const char *what) {
        if (!on) return;
        const auto t = clk::now();
        if (len < (int)sizeof buf - 40) len += snprintf(buf + len, sizeof buf - len, " %s %.0f", what, us(t - last));
        last = t;
    }
    ~HostMarks() {
        if (!on) return;
        cur() = prev;
        fprintf(stderr, "[gf] host us:%s | total %.0f\n", buf, us(clk::now() - t0));
    }
};
void host_mark(const char *what) { if (HostMarks *m = HostMarks::cur()) m->mark(what); }
// ---- call contexts: the device workspaces of one classify call.  Each HIP
// stream has its own, so calls on different streams (over disjoint programs and
// maps, see CallOrder) run concurrently, host and device; calls on one stream
// take its context one at a time.  Workspace accessors keep one instance of
// their type per context (CallCtx::get).
}  // namespace
namespace gf {
struct CallCtx {
    std::mutex mu;
    hipEvent_t ev = nullptr;       // recorded at the end of every call in this context (made with the context)
    std::atomic<bool> have{false}; // ev has been recorded once (read by other contexts' CallOrder)
    int ws_slot = 0;      // gf_policy_ingress_classify_batches: schedule k+1 builds in one while k runs
    std::map<const void *, std::shared_ptr<void>> bag;
    template <class T> T &get(const void *tag) {
        auto &p = bag[tag];
        if (!p) p = std::make_shared<T>();
        return *static_cast<T *>(p.get());
    }
};
}  // namespace gf
namespace {
thread_local CallCtx *t_ctx = nullptr;
CallCtx &ctx_for(hipStream_t s) {
    static std::mutex mu;
    static std::map<hipStream_t, std::unique_ptr<CallCtx>> all;
    std::lock_guard<std::mutex> g(mu);
    auto &c = all[s];
    if (!c) {
        c = std::make_unique<CallCtx>();
        // the call-order event exists before any other thread can see the context
        // (device-scope release: the event orders device work between streams)
        if (hipEventCreateWithFlags(&c->ev, hipEventDisableTiming | hipEventReleaseToDevice) != hipSuccess) c->ev = nullptr;
    }
    return *c;
}
// The calling thread's context (map API paths outside a classify call: the
// null stream's).
CallCtx &cur_ctx() { return t_ctx ? *t_ctx : ctx_for(nullptr); }
struct CtxScope {
    CallCtx *prev, *c;
    std::unique_lock<std::mutex> l;
    explicit CtxScope(hipStream_t s) : prev(t_ctx), c(&ctx_for(s)), l(c->mu) { t_ctx = c; }
    ~CtxScope() { t_ctx = prev; }
};
Workspace &ws() {
    static const char tag = 0;
    CallCtx &c = cur_ctx();
    struct Two { Workspace w[2]; };
    return c.get<Two>(&tag).w[c.ws_slot];
}
gf_event_ring &event_ring() { static gf_event_ring r{}; return r; }
struct PipeWs {
    DevBuf s6, d6;             // IPv6 addresses of the rewritten frames (read by handle_policy)
};
PipeWs &pipe_ws() { static const char tag = 0; return cur_ctx().get<PipeWs>(&tag); }

int check_cols(const gf_pkt_cols *p) {
    if (!p) return -EFAULT;
    if (p->n == 0) return 0;
    if (!p->len || !p->ethertype || !p->saddr4 || !p->daddr4 || !p->proto || !p->l4_off || !p->l4w0 || !p->l4w3)
        return -EFAULT;
    return 1;
}

uint32_t grid_for(uint32_t n) {
    uint32_t g = (n + BLOCK - 1) / BLOCK;
    return g < 1 ? 1 : (g > 65535u * 8 ? 65535u * 8 : g);
}
// Grid of the one-packet-per-lane stream kernels (k_xdp, k_lb): capped at
// GF_STREAM_GRID blocks (grid-stride beyond) so the per-block counter flush
// stays a few thousand atomics per bin; 0 = one lane per packet.  Measured
// (config 3, k_lb, 16M packets): uncapped 0.86 ms, 2k 0.85, 4k 0.72, 16k 0.68.
#ifndef GF_STREAM_GRID
#define GF_STREAM_GRID 16384
#endif
// GPUFLOW_STREAM_GRID overrides the cap (the GPU tests force a few blocks so
// every block runs several tiles of the grid-stride loop).
uint32_t stream_grid_cap() {
    const char *e = getenv("GPUFLOW_STREAM_GRID");
    return e ? (uint32_t)strtoul(e, nullptr, 10) : (uint32_t)GF_STREAM_GRID;
}
uint32_t stream_grid(uint32_t n, uint32_t per_block = BLOCK) {
    const uint32_t g = n == 0 ? 1u : (n + per_block - 1) / per_block, cap = stream_grid_cap();
    const uint32_t lim = cap ? cap : 65535u * 8;      // grid-stride covers the rest
    return g > lim ? lim : g;
}

int push_map(const std::shared_ptr<Map> &m, hipStream_t s) { return m ? m->push(s) : 0; }
// bpf_lb's launch descriptor: the service maps (pushed by the caller) and the program's flags
LbDev lb_dev(const ProgLb &p) {
    LbDev L{};
    if (p.lb4) L.s4 = p.lb4->hdesc();
    if (p.lb6) L.s6 = p.lb6->hdesc();
    L.flags = p.cfg.flags;
    return L;
}
// The v4 prefixes as DIR-24-8 tables for XdpDev (GF_XDP_DIR24=1: the A/B against
// the trie walk), when they build.
void xdp_dir(const std::shared_ptr<Map> &l4, XdpDev &x, hipStream_t s) {
    const char *e = getenv("GF_XDP_DIR24");       // read per call: a test flips it in-process
    const bool on = e && atoi(e) != 0;
    x.d24 = nullptr; x.d8 = nullptr;
    if (on && l4 && l4->dir24(s, &x.d24, &x.d8)) { x.d24 = nullptr; x.d8 = nullptr; }
}
// The prefilter's compact address sets (Map::addr_set) for XdpDev, when they build.
void xdp_sets(const std::shared_ptr<Map> &h4, const std::shared_ptr<Map> &lxc, XdpDev &x, hipStream_t s) {
    static const bool no_sets = getenv("GF_XDP_NOSETS") != nullptr;     // diagnosis: the hash tables
    if (no_sets) return;
    if (h4 && h4->addr_set(8, 8192, s, &x.h4set, &x.h4bits, &x.h4zero)) x.h4set = nullptr;
    if (lxc && lxc->addr_set(20, 8192, s, &x.lxset, &x.lxbits, &x.lxzero)) x.lxset = nullptr;
}

// ---- device-side order of the calls that share an object.  Every map a call
// binds and the cilium_policy array it runs remember the call context (stream)
// of the last call that used them (OrderPt): a call first waits on the end event
// of each other context found there (one wait per context, on its latest call —
// a conservative bound), so a kernel still reading or writing a map replica (or a
// program table) finishes before this call pushes into it or runs over it; at its
// end the call records its context's event once and marks every object with its
// context (under the objects' locks).  The workspaces are per stream (CallCtx), so
// calls over disjoint objects on different streams do not wait on each other.
// With an event ring set, calls append to it in turn.
std::mutex &ring_mu() { static std::mutex m; return m; }
OrderPt &ring_ord() { static OrderPt o; return o; }
struct CallOrder {
    hipStream_t s;
    CallCtx *me;
    std::vector<OrderPt *> pts;
    std::unique_lock<std::mutex> ring;
    CallOrder(hipStream_t s_, std::vector<OrderPt *> p) : s(s_), me(&cur_ctx()), pts(std::move(p)) {
        if (event_ring().records) {
            ring = std::unique_lock<std::mutex>(ring_mu());
            pts.push_back(&ring_ord());
        }
        CallCtx *waited[8];
        int nw = 0;
        for (OrderPt *o : pts) {
            CallCtx *c = o->last;
            if (!c || c == me || !c->have.load(std::memory_order_acquire)) continue;
            bool seen = false;
            for (int k = 0; k < nw; k++) seen |= waited[k] == c;
            if (seen) continue;
            (void)hipStreamWaitEvent(s, c->ev, 0);
            if (nw < 8) waited[nw++] = c;
        }
    }
    CallOrder(hipStream_t s_, const MapLocks &L, PolicyArray *a = nullptr) : CallOrder(s_, order_pts(L, a)) {}
    static std::vector<OrderPt *> order_pts(const MapLocks &L, PolicyArray *a) {
        std::vector<OrderPt *> v;
        for (Map *m : L.held) v.push_back(&m->ord);
        if (a) v.push_back(&a->ord);
        return v;
    }
    ~CallOrder() {
        if (!me->ev || hipEventRecord(me->ev, s) != hipSuccess) return;
        me->have.store(true, std::memory_order_release);
        for (OrderPt *o : pts) o->last = me;
    }
};
void lock_lxc_maps(MapLocks &L, const std::shared_ptr<ProgLxc> &p) {
    for (auto m : {p->policy, p->ct4, p->ct6, p->cidr4, p->cidr6, p->revnat4, p->revnat6, p->lb4, p->ipcache,
                   p->cidr4e, p->lb6, p->cidr6e})
        L.add(m);
}
void lock_array_maps(MapLocks &L, const std::shared_ptr<PolicyArray> &a) {
    for (auto &kv : a->slots) lock_lxc_maps(L, kv.second);
    L.add(proxy_map(4)); L.add(proxy_map(6)); L.add(node_map(1)); L.add(node_map(2));
}
void lock_xdp_maps(MapLocks &L, const ProgXdp &x) { L.add(x.m4h); L.add(x.m4l); L.add(x.m6h); L.add(x.m6l); L.add(x.lxc); }


// blocks of BLOCK threads that fill the device at `per_cu` blocks per CU
uint32_t resident_blocks(uint32_t per_cu) {
    static const int cus = [] {                   // thread-safe one-time init (concurrent calls)
        int dev = 0, c = 0;
        if (hipGetDevice(&dev) != hipSuccess ||
            hipDeviceGetAttribute(&c, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || c <= 0)
            c = 256;
        return c;
    }();
    return (uint32_t)cus * per_cu;
}

}  // namespace
