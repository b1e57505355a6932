"""The reference programs executed as host code — TEST INFRASTRUCTURE ONLY.

Generates the config headers a reference program needs for a synth.Scenario, compiles
the wrapper units of oracle/ref/ against the reference checkout (reached only by -I and
#include name) into oracle/_ref/, runs them through oracle/_ref/ref_runner and reads back
what every packet left behind.  oracle/REFDIFF.md says how those observables map onto the
records of libgpuflow and of the CPU oracle; tests/golden/make_ref_golden.py records them.

The reference checkout is found through $GF_REFERENCE (default: the location oracle.h
cites).  Without one, build() does nothing and has_runner() stays False.
"""
import hashlib
import json
import os
import struct
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "ref")
OUT = os.path.join(HERE, "_ref")
RUNNER = os.path.join(OUT, "ref_runner")
REF_ENV = "GF_REFERENCE"
REF_DEFAULT = "/root/reference"
CC = os.environ.get("CC", "gcc")
CFLAGS = ["-O1", "-g", "-fPIC", "-fvisibility=hidden", "-w", "-D__NR_CPUS__=1", "-U_FORTIFY_SOURCE"]

TC_ACT_OK, TC_ACT_SHOT, TC_ACT_REDIRECT = 0, 2, 7
NOT_RUN = -(1 << 31) + 1          # no program in the packet's cilium_policy slot
LEFT = -(1 << 31)                 # left through a recorded tail call
DROP_MISSED_TAIL_CALL = 140
OBS = np.dtype([("ret", "<i4"), ("redirect_called", "<u4"), ("redirect_ifindex", "<u4"), ("redirect_flags", "<u4"),
                ("tail_called", "<u4"), ("tail_map", "<u4"), ("tail_index", "<u4"), ("cb", "<u4", (5,)),
                ("unmodelled", "<u4")])


def reference_root():
    p = os.environ.get(REF_ENV, REF_DEFAULT)
    return p if os.path.isfile(os.path.join(p, "bpf", "bpf_lxc.c")) else None


def has_runner():
    return os.path.isfile(RUNNER)


# ------------------------------------------------------------------ config headers
def _bytes(b, n):
    b = bytes(b or bytes(n))
    return ", ".join(hex(x) for x in b)


def _mac(b):
    return "{ .addr = { %s } }" % _bytes(b, 6)


def _swap16(x):
    return ((x & 0xff) << 8) | (x >> 8)


def _swap32(x):
    return int.from_bytes((x & 0xffffffff).to_bytes(4, "little"), "big")


def node_config(sc):
    nd = sc.node or {}
    return "\n".join([
        "/* generated for scenario %s: node_config.h */" % sc.name,
        "#define ROUTER_IP %s" % _bytes(nd.get("router_ip6"), 16),
        "#define HOST_IFINDEX %d" % sc.host_ifindex,
        "#define HOST_IP %s" % _bytes(nd.get("host_ip6"), 16),
        "#define HOST_ID 1", "#define WORLD_ID 2", "#define CLUSTER_ID 3",
        "#define HOST_IFINDEX_MAC %s" % _mac(nd.get("host_mac")),
        "#define NODE_MAC %s" % _mac(nd.get("node_mac")),
        "#define NAT46_PREFIX { .addr = { 0 } }",
        "#define IPV4_MASK %#x" % nd.get("ipv4_mask", 0xffff),
        "#define IPV4_CLUSTER_MASK %#x" % nd.get("ipv4_cluster_mask", 0xff0000),
        "#define IPV4_CLUSTER_RANGE %#x" % nd.get("ipv4_cluster_range", 0x100000),
        "#define IPV4_GATEWAY %#x" % nd.get("ipv4_gateway", 0),
        "#define IPV4_LOOPBACK %#x" % nd.get("ipv4_loopback", 0),
        "#define ENABLE_IPV4", "#define LB_RR_MAX_SEQ 31",
        "#define TUNNEL_ENDPOINT_MAP_SIZE 65536", "#define ENDPOINTS_MAP_SIZE 65536",
        "#define CILIUM_LB_MAP_MAX_ENTRIES 65536", "#define PROXY_MAP_SIZE 524288",
        "#define POLICY_MAP_SIZE 16384", "#define IPCACHE_MAP_SIZE 512000",
        "#define POLICY_PROG_MAP_SIZE ENDPOINTS_MAP_SIZE",
        "#define HAVE_LRU_MAP_TYPE", "#define HAVE_LPM_MAP_TYPE", ""])


def _maps_macro(rows):
    return "#define REF_MAPS " + " ".join('X(%s, "%s")' % (obj, name) for obj, name in rows if name)


def lxc_config(sc, e):
    """lxc_config.h of one endpoint program (pkg/endpoint/bpf.go writes the real one)."""
    fl = e["flags"]
    if fl & ~0xdf:
        raise ValueError("endpoint option outside the harness: flags %#x" % fl)
    nd = sc.node or {}
    i = e["lxc_id"]
    L = ["/* generated for scenario %s, endpoint %d: lxc_config.h */" % (sc.name, i),
         "#define LXC_MAC %s" % _mac(e.get("lxc_mac")),
         "#define LXC_IP %s" % _bytes(e.get("lxc_ip6"), 16),
         "#define LXC_ID %d" % i, "#define LXC_ID_NB %#x" % _swap16(i),
         "#define SECLABEL %d" % e["seclabel"], "#define SECLABEL_NB %#x" % _swap32(e["seclabel"]),
         "#define POLICY_MAP cilium_policy_%d" % i, "#define CALLS_MAP cilium_calls_%d" % i,
         "#define CT_MAP4 cilium_ct4_%d" % i, "#define CT_MAP6 cilium_ct6_%d" % i,
         "#define CT_MAP_SIZE %d" % sc.maps[e["ct4"]].max_entries if e.get("ct4") else "#define CT_MAP_SIZE 4096",
         "#define DROP_NOTIFY", "#define LB_L3", "#define LB_L4"]
    if fl & 1:
        L.append("#define DROP_ALL")
    if fl & 2:
        L.append("#define POLICY_INGRESS")
    if fl & 4:
        L.append("#define HAVE_L4_POLICY")
    if fl & 8:
        L.append("#define CONNTRACK_ACCOUNTING")
    if fl & 16:
        L.append("#define LXC_IPV4 %#x" % e.get("lxc_ipv4", 0))
    if fl & 64:
        L.append("#define TRACE_NOTIFY")
    if not fl & 128:
        L.append("#define CONNTRACK")
    l4 = e.get("l4") or []
    if l4:
        rows = ", ".join("%d, %d, %d, %d" % (k, _swap16(p), _swap16(x), nh) for k, (p, x, nh) in enumerate(l4))
        L.append("#define CFG_L3L4_INGRESS %s, (), 0" % rows)
    binds = [("CT_MAP4", e.get("ct4")), ("CT_MAP6", e.get("ct6")), ("POLICY_MAP", e.get("policy")),
             ("cilium_lb4_reverse_nat", e.get("revnat4")), ("cilium_lb6_reverse_nat", e.get("revnat6")),
             ("cilium_proxy4", nd.get("proxy4")), ("cilium_proxy6", nd.get("proxy6"))]
    if fl & 2:
        if e.get("cidr4"):
            L.append("#define CIDR4_INGRESS_MAP cilium_cidr4_ingress_%d" % i)
            binds.append(("CIDR4_INGRESS_MAP", e["cidr4"]))
        if e.get("cidr6"):
            L.append("#define CIDR6_INGRESS_MAP cilium_cidr6_ingress_%d" % i)
            binds.append(("CIDR6_INGRESS_MAP", e["cidr6"]))
    L += ["#define REF_ENTRY handle_policy", _maps_macro(binds), ""]
    return "\n".join(L)


def lb_config(sc):
    lb = sc.lb
    fl = lb["flags"]
    L = ["/* generated for scenario %s: netdev_config.h of bpf_lb */" % sc.name, "#define DROP_NOTIFY",
         "#define CALLS_MAP cilium_calls_lb"]
    if fl & 1:
        L.append("#define LB_L3")
    if fl & 2:
        L.append("#define LB_L4")
    if fl & 4:
        L.append("#define LB_REDIRECT %d" % lb.get("redirect_ifindex", 0))
    if fl & 8:
        L.append("#define LB_DISABLE_IPV4")
    if fl & 16:
        L.append("#define LB_DISABLE_IPV6")
    if lb.get("dstmac") is not None:
        L.append("#define LB_DSTMAC %s" % _mac(lb["dstmac"]))
    L += ["#define REF_ENTRY from_netdev",
          _maps_macro([("cilium_lb4_services", lb.get("lb4")), ("cilium_lb6_services", lb.get("lb6"))]), ""]
    return "\n".join(L)


def programs(sc, program):
    """[(slot, wrapper unit, {header name: text})] of a scenario's `program` ('lxc' or 'lb')."""
    node = node_config(sc)
    if program == "lxc":
        return [(e["lxc_id"], "ref_bpf_lxc.c", {"node_config.h": node, "lxc_config.h": lxc_config(sc, e)})
                for e in sc.lxc]
    if program == "lb":
        return [(0, "ref_bpf_lb.c", {"node_config.h": node, "netdev_config.h": lb_config(sc)})]
    raise ValueError(program)


def _cfg_dir(unit, headers):
    h = hashlib.sha256(unit.encode())
    for k in sorted(headers):
        h.update(k.encode() + b"\0" + headers[k].encode() + b"\0")
    for f in ("ref_shim.h", "ref_rt.h", unit):
        with open(os.path.join(SRC, f), "rb") as fh:
            h.update(fh.read())
    return os.path.join(OUT, "cfg_" + h.hexdigest()[:16])


# ------------------------------------------------------------------ the recipe
def _run(cmd):
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode:
        raise RuntimeError("%s\n%s" % (" ".join(cmd), r.stderr[-4000:]))


def build_runner(sanitize=False):
    os.makedirs(OUT, exist_ok=True)
    exe = RUNNER + ("_san" if sanitize else "")
    src = os.path.join(SRC, "ref_runner.c")
    deps = [src, os.path.join(SRC, "ref_rt.h")]
    if os.path.exists(exe) and all(os.path.getmtime(exe) >= os.path.getmtime(d) for d in deps):
        return exe
    san = ["-fsanitize=address,undefined", "-fno-omit-frame-pointer"] if sanitize else []
    _run([CC, "-O1", "-g", "-Wall", "-Wextra", *san, "-I", SRC, src, "-o", exe, "-ldl"])
    return exe


def build_program(unit, headers, sanitize=False):
    """One wrapper unit with its generated headers -> oracle/_ref/cfg_<hash>/prog.so."""
    d = _cfg_dir(unit, headers)
    so = os.path.join(d, "prog_san.so" if sanitize else "prog.so")
    if os.path.exists(so):
        return so
    root = reference_root()
    if root is None:
        raise RuntimeError("no reference checkout (set $%s)" % REF_ENV)
    os.makedirs(d, exist_ok=True)
    for k, text in headers.items():
        with open(os.path.join(d, k), "w") as f:
            f.write(text)
    bpf = os.path.join(root, "bpf")
    san = ["-fsanitize=address,undefined", "-fno-omit-frame-pointer"] if sanitize else []
    tmp = so + ".tmp%d" % os.getpid()
    _run([CC, *CFLAGS, *san, "-shared", "-Wl,-Bsymbolic", "-I", d, "-I", os.path.join(bpf, "include"), "-I", bpf,
          "-I", SRC, os.path.join(SRC, unit), "-o", tmp])
    os.replace(tmp, so)
    return so


def build(cases=None, sanitize=False):
    """The runner and every program object of the committed cases.  No reference tree: nothing."""
    if reference_root() is None:
        return False
    from concurrent.futures import ThreadPoolExecutor
    from . import ref_cases
    build_runner(sanitize)
    jobs = {}
    for name in (cases or ref_cases.CASES):
        sc = ref_cases.scenario(name)
        for program in ref_cases.PROGRAMS:
            for _, unit, headers in programs(sc, program):
                jobs[_cfg_dir(unit, headers)] = (unit, headers)
    with ThreadPoolExecutor(min(8, os.cpu_count() or 1)) as ex:
        list(ex.map(lambda j: build_program(j[0], j[1], sanitize), jobs.values()))
    return True


# ------------------------------------------------------------------ input / output files
def _col(x, n):
    return np.zeros(n, "<u4") if x is None else np.ascontiguousarray(x).astype("<u4")


def input_bytes(sc, program, nows, objects, seed=0x5eed):
    """The runner's flat input: seed, routing, maps, program objects, batches."""
    out = [struct.pack("<IQI", 0x49524647, seed, 1 if program == "lxc" else 0), struct.pack("<I", len(sc.maps))]
    for name, m in sc.maps.items():
        n = m.n()
        out.append(struct.pack("<32s5I", name.encode(), m.type, m.ksz, m.vsz, m.max_entries, n))
        if n:
            out.append(np.ascontiguousarray(m.keys, np.uint8).tobytes())
            out.append(np.ascontiguousarray(m.vals, np.uint8).tobytes())
    out.append(struct.pack("<I", len(objects)))
    for slot, path in objects:
        out.append(struct.pack("<I512s", slot, path.encode()))
    out.append(struct.pack("<I", len(sc.batches)))
    for pk, now in zip(sc.batches, nows):
        n = pk.n
        out.append(struct.pack("<IIQ", n, pk.frames.shape[1], int(now) * 1_000_000_000))
        out.append(np.ascontiguousarray(pk.frames, np.uint8).tobytes())
        for c in (pk.lens, pk.src_identity, pk.ifindex, pk.lxc_id, pk.tc_index, pk.flow_hash, pk.mark):
            out.append(_col(c, n).tobytes())
    return b"".join(out)


def input_digest(sc, program, nows):
    """sha256 of what the runner is fed: the input file with the object paths left out,
    plus the generated headers."""
    h = hashlib.sha256(input_bytes(sc, program, nows, []))
    for slot, unit, headers in programs(sc, program):
        h.update(struct.pack("<I", slot) + unit.encode())
        for k in sorted(headers):
            h.update(headers[k].encode())
    return h.hexdigest()


def read_output(buf):
    """-> (bind names, [per batch {obs, frames, ev_off, ev, maps{name: (keys, vals)}}])."""
    o = 0

    def take(fmt):
        nonlocal o
        v = struct.unpack_from(fmt, buf, o)
        o += struct.calcsize(fmt)
        return v

    def arr(dt, count, shape=None):
        nonlocal o
        a = np.frombuffer(buf, dt, count, o).copy()
        o += a.nbytes
        return a if shape is None else a.reshape(shape)

    magic, nb = take("<II")
    assert magic == 0x4f524647
    binds = [take("<32s")[0].rstrip(b"\0").decode() for _ in range(nb)]
    batches = []
    for _ in range(take("<I")[0]):
        n, stride = take("<II")
        b = {"obs": arr(OBS, n), "frames": arr(np.uint8, n * stride, (n, stride)), "ev_off": arr("<u4", n + 1)}
        b["ev"] = arr(np.uint8, int(b["ev_off"][-1]))
        b["maps"] = {}
        for _ in range(take("<I")[0]):
            name, ksz, vsz, cnt = take("<32s3I")
            k = arr(np.uint8, cnt * ksz, (cnt, ksz))
            v = arr(np.uint8, cnt * vsz, (cnt, vsz))
            b["maps"][name.rstrip(b"\0").decode()] = (k, v)
        batches.append(b)
    assert o == len(buf)
    return binds, batches


def run(sc, program, nows, sanitize=False):
    """Builds what is missing, runs the scenario's batches through `program`, returns read_output()."""
    exe = build_runner(sanitize)
    objs = [(slot, build_program(unit, headers, sanitize)) for slot, unit, headers in programs(sc, program)]
    with tempfile.TemporaryDirectory() as d:
        fi, fo = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
        with open(fi, "wb") as f:
            f.write(input_bytes(sc, program, nows, objs))
        r = subprocess.run([exe, "run", fi, fo], capture_output=True, text=True)
        if r.returncode:
            raise RuntimeError("ref_runner exit %d\n%s" % (r.returncode, r.stderr[-4000:]))
        with open(fo, "rb") as f:
            return read_output(f.read())


def csum_run(records, sanitize=False):
    """The shim's checksum helpers on [(op, a, b, c, d, buf64)] -> [(ret, buf64)]."""
    exe = build_runner(sanitize)
    with tempfile.TemporaryDirectory() as d:
        fi, fo = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
        with open(fi, "wb") as f:
            f.write(struct.pack("<I", len(records)))
            for op, a, b, c, dd, buf in records:
                f.write(struct.pack("<5I64s", op, a, b, c, dd, bytes(buf)))
        subprocess.run([exe, "csum", fi, fo], check=True)
        with open(fo, "rb") as f:
            raw = f.read()
    return [struct.unpack_from("<i64s", raw, 68 * i) for i in range(len(records))]


# ------------------------------------------------------------------ fixtures
def written_maps(sc, program):
    """The maps `program` writes (dumped per batch): CT, policy counters, proxy entries."""
    if program != "lxc":
        return []
    nd = sc.node or {}
    names = [nd.get("proxy4"), nd.get("proxy6")]
    for e in sc.lxc:
        names += [e.get("ct4"), e.get("ct6"), e.get("policy")]
    return sorted({n for n in names if n})


def fixture_arrays(sc, program, nows, params):
    """What tests/golden/ref_<program>_<case>.npz holds."""
    binds, batches = run(sc, program, nows)
    keep = written_maps(sc, program)
    d = {"params": np.frombuffer(json.dumps(params, sort_keys=True).encode(), np.uint8),
         "input_sha": np.frombuffer(input_digest(sc, program, nows).encode(), np.uint8),
         "binds": np.frombuffer("\n".join(binds).encode(), np.uint8), "maps": np.frombuffer("\n".join(keep).encode(), np.uint8)}
    for i, b in enumerate(batches):
        d["b%d_obs" % i] = b["obs"].view("<u4").reshape(len(b["obs"]), -1)
        d["b%d_frames" % i] = b["frames"]
        d["b%d_ev_off" % i] = b["ev_off"]
        d["b%d_ev" % i] = b["ev"]
        for name in keep:
            d["b%d_map_%s_k" % (i, name)], d["b%d_map_%s_v" % (i, name)] = b["maps"][name]
    return d


def load_fixture(path):
    z = np.load(path)
    s = lambda k: bytes(z[k]).decode()
    fx = {"params": json.loads(s("params")), "input_sha": s("input_sha"), "binds": s("binds").split("\n"),
          "maps": [m for m in s("maps").split("\n") if m], "batches": []}
    i = 0
    while "b%d_obs" % i in z.files:
        b = {"obs": np.ascontiguousarray(z["b%d_obs" % i]).view(OBS).reshape(-1), "frames": z["b%d_frames" % i],
             "ev_off": z["b%d_ev_off" % i], "ev": z["b%d_ev" % i],
             "maps": {m: (z["b%d_map_%s_k" % (i, m)], z["b%d_map_%s_v" % (i, m)]) for m in fx["maps"]}}
        fx["batches"].append(b)
        i += 1
    return fx


# ------------------------------------------------------------------ the REFDIFF.md mapping
def events_160(b, stride=None):
    """A batch's events as the 160-byte ring records (32-byte header + up to 128 captured
    bytes, zero padded), in emission order, with the packet index of each."""
    recs, owner = [], []
    ev, off = b["ev"], b["ev_off"]
    for i in range(len(off) - 1):
        o, end = int(off[i]), int(off[i + 1])
        while o < end:
            msz, cap = struct.unpack_from("<II", ev, o)
            r = np.zeros(160, np.uint8)
            assert msz == 32 and cap <= 128
            r[:32 + cap] = ev[o + 8:o + 8 + 32 + cap]
            if stride is not None and cap > stride:
                r[32 + stride:] = 0              # bytes past the snap are not held by the batch
            recs.append(r)
            owner.append(i)
            o += 8 + msz + cap
    return np.array(recs, np.uint8).reshape(-1, 160), np.array(owner, np.int64)


def ingress_records(b, pk, host_ifindex, l4_off):
    """gf_ingress_out fields that the reference's observables define (REFDIFF.md):
    action, reason, flags bit 0, proxy_port, ifindex_lo.  l4_off: where the L4 header starts
    (plain_l4_off), used only to find the destination port in the frame a proxy redirect left."""
    obs = b["obs"]
    n = len(obs)
    ret = obs["ret"]
    run_ = ret != NOT_RUN
    assert not np.any(ret == LEFT)
    action = np.where(run_, ret, TC_ACT_SHOT).astype(np.uint8)
    shot = action == TC_ACT_SHOT
    reason = np.where(run_, (-obs["cb"][:, 2].astype(np.int32)) & 0xff, DROP_MISSED_TAIL_CALL)
    reason = np.where(shot, reason, 0).astype(np.uint8)
    redir = (ret == TC_ACT_REDIRECT) & (obs["redirect_called"] == 1)
    assert np.array_equal(ret == TC_ACT_REDIRECT, redir)
    ifx = np.where(redir, obs["redirect_ifindex"] & 0xffff, 0).astype(np.uint16)
    in_ifx = _col(pk.ifindex, n)
    proxied = redir & (obs["redirect_ifindex"] == host_ifindex) & (in_ifx != host_ifindex)
    fr = b["frames"]
    po = np.clip(l4_off.astype(np.int64) + 2, 0, fr.shape[1] - 2)
    rows = np.arange(n)
    dport = fr[rows, po].astype(np.uint16) | (fr[rows, po + 1].astype(np.uint16) << 8)
    return {"action": action, "reason": reason, "proxied": proxied.astype(np.uint8),
            "proxy_port": np.where(proxied, dport, 0).astype(np.uint16), "ifindex_lo": ifx}


def plain_l4_off(pk):
    """The L4 offset of the frames whose L4 header directly follows a plain IP header, from the
    frame bytes alone: IPv4 14 + IHL * 4 with IHL >= 5, IPv6 54 with TCP or UDP as the first next
    header; -1 elsewhere (extension headers, short IHL, other ethertypes)."""
    f = pk.frames
    v4 = (f[:, 12] == 0x08) & (f[:, 13] == 0x00)
    v6 = (f[:, 12] == 0x86) & (f[:, 13] == 0xDD)
    ihl = (f[:, 14] & 0xf).astype(np.int64)
    off = np.full(pk.n, -1, np.int64)
    off = np.where(v4 & (ihl >= 5), 14 + 4 * ihl, off)
    off = np.where(v6 & ((f[:, 20] == 6) | (f[:, 20] == 17)), 54, off)
    return off


def lb_records(b, pk):
    """gf_lb_out fields that the reference's observables define: action, reason, and, for a
    translated frame, new_daddr4 / new_daddr6 as the frame holds them."""
    obs = b["obs"]
    ret = obs["ret"]
    action = ret.astype(np.uint8)
    shot = ret == TC_ACT_SHOT
    reason = np.where(shot, (-obs["cb"][:, 2].astype(np.int32)) & 0xff, 0).astype(np.uint8)
    fr = b["frames"]
    return {"action": action, "reason": reason, "daddr4": np.ascontiguousarray(fr[:, 30:34]).view("<u4").ravel(),
            "daddr6": fr[:, 38:54]}
