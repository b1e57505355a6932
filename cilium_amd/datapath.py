"""Host side of the datapath: load programs over maps and run classify calls.

This mirrors what the agent does in the reference: create/pin maps through
pkg/bpf (here cilium_amd.bpf over libgpuflow), generate the per-endpoint
configuration (pkg/endpoint/bpf.go:156-330 -> gf_lxc_cfg instead of a
compiled header), install the tail-call slots (cilium_policy prog array) and
then let packets flow — here, batches resident in HBM.

Batches are torch tensors on the current CUDA/HIP device; PyTorch is only the
allocator/stream provider, every computation runs in libgpuflow's kernels.
"""
import ctypes as C
import errno

import numpy as np

from . import bpf
from .maps import ctmap
from ._lib import (lib, gf_frames, gf_pkt_cols, gf_pkt_cols_out, gf_xdp_cfg, gf_xdp_frames_out, gf_lb_cfg, gf_lxc_cfg,
                   gf_node_cfg, gf_netdev_cfg, gf_pipeline_cfg, gf_pipe_batch, gf_lxc_batch, gf_overlay_cfg,
                   gf_overlay_batch, gf_tunnel_opts, gf_host_cfg, gf_host_batch, gf_respond_cfg, gf_respond_batch,
                   gf_tunnel_cfg, gf_tunnel_tx, gf_tunnel_rx_out, GF_TUN_GENEVE,
                   gf_event_ring, gf_event_drain_out, GF_EVENT_RECORD, GF_EVD_F_PACKED, GF_EVD_F_RESET, GF_EVD_MAX_WINDOW,
                   GF_CALL_ICMP6_TIME_EXCEEDED, GF_REC_EGRESS, GF_REC_PIPELINE,
                   gf_forward_cfg, gf_forward_ifindex, gf_forward_out, GF_FWD_DROP)

LB_OUT = np.dtype([("action", "u1"), ("reason", "u1"), ("slave", "<u2"), ("new_dport", "<u2"),
                   ("rev_nat", "<u2"), ("new_daddr4", "<u4")])
ING_OUT = np.dtype([("action", "u1"), ("reason", "u1"), ("ct_ret", "u1"), ("flags", "u1"),
                    ("proxy_port", "<u2"), ("ifindex_lo", "<u2")])
PIPE_OUT = np.dtype([("stage", "u1"), ("action", "u1"), ("reason", "u1"), ("ct_ret", "u1"), ("flags", "u1"),
                     ("pad0", "u1"), ("proxy_port", "<u2"), ("ifindex_lo", "<u2"), ("slave", "<u2"),
                     ("rev_nat", "<u2"), ("dport", "<u2"), ("daddr4", "<u4"), ("lxc_id", "<u2"), ("pad1", "<u2")])
EG_OUT = np.dtype([("stage", "u1"), ("action", "u1"), ("reason", "u1"), ("ct_ret", "u1"), ("flags", "u1"),
                   ("eg_ct_ret", "u1"), ("proxy_port", "<u2"), ("ifindex_lo", "<u2"), ("slave", "<u2"),
                   ("rev_nat", "<u2"), ("eg_flags", "<u2"), ("tunnel_ip", "<u4"), ("lxc_id", "<u2"), ("pad", "<u2")])


def _be16(x):
    return ((x & 0xff) << 8) | (x >> 8)


def egress_fields(c, e, h):
    """The from-container section of an endpoint's gf_lxc_cfg (pkg/endpoint/bpf.go:156-330
    emits these as LXC_MAC, NODE_MAC, LXC_IPV4, LXC_PORT_MAPPINGS, CFG_L3L4_EGRESS)."""
    c.lxc_mac[:] = list(e.get("lxc_mac", bytes(6)))
    c.node_mac[:] = list(e.get("node_mac", bytes(6)))
    c.lxc_ipv4 = e.get("lxc_ipv4", 0)
    c.lb4_services, c.ipcache_map, c.cidr4_egress_map = h(e.get("lb4")), h(e.get("ipcache")), h(e.get("cidr4e"))
    c.lb6_services, c.cidr6_egress_map = h(e.get("lb6")), h(e.get("cidr6e"))
    c.lxc_ip6[:] = list(e.get("lxc_ip6", bytes(16)))
    pm = e.get("portmap") or []
    c.n_portmap = len(pm)
    for i, (frm, to) in enumerate(pm):
        c.portmap[2 * i], c.portmap[2 * i + 1] = _be16(frm), _be16(to)
    l4 = e.get("l4e") or []
    c.n_l4_egress = len(l4)
    for i, (port, proxy, nh) in enumerate(l4):
        c.l4_egress[i].port, c.l4_egress[i].proxy, c.l4_egress[i].nexthdr = _be16(port), _be16(proxy), nh


def _torch():
    import torch
    return torch


def _check(rc, what):
    if rc < 0:
        raise OSError(-rc, f"{what}: {errno.errorcode.get(-rc, rc)}")
    return rc


def _ptr(t):
    return None if t is None else t.data_ptr()


def _stream():
    torch = _torch()
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class DeviceBatch:
    """Raw frames + skb metadata uploaded to HBM, parsed into SoA columns by
    gf_parse_frames (k_parse)."""

    def __init__(self, pk, device="cuda", parse=True, with_v6=True):
        torch = _torch()
        self.n = pk.n
        self.device = device
        signed = {np.dtype(np.uint32): np.int32, np.dtype(np.uint16): np.int16, np.dtype(np.uint8): np.uint8}

        def t(a, dt):
            if a is None:
                return None
            a = np.ascontiguousarray(np.asarray(a).astype(dt, copy=False))
            return torch.from_numpy(a.view(signed[np.dtype(dt)])).to(device)

        self.frames = t(pk.frames, np.uint8)
        self.len = t(pk.lens, np.uint32)
        self.src_identity = t(pk.src_identity, np.uint32)
        self.ifindex = t(pk.ifindex, np.uint32)
        self.lxc_id = t(pk.lxc_id, np.uint16)
        self.tc_index = t(pk.tc_index, np.uint8)
        self.flow_hash = t(pk.flow_hash, np.uint32)
        self.tunnel_id = t(getattr(pk, "tunnel_id", None), np.uint32)   # bpf_tunnel_key.tunnel_id (from-overlay)
        self.mark = t(getattr(pk, "mark", None), np.uint32)             # skb->mark (from-host)
        n = self.n
        e = lambda dt, *shape: torch.empty((n,) + shape, dtype=dt, device=device)
        self.ethertype = e(torch.int16)
        self.saddr4 = e(torch.int32)
        self.daddr4 = e(torch.int32)
        self.proto = e(torch.uint8)
        self.l4_off = e(torch.int16)
        self.l4w0 = e(torch.int32)
        self.l4w3 = e(torch.int16)
        self.saddr6 = e(torch.uint8, 16) if with_v6 else None
        self.daddr6 = e(torch.uint8, 16) if with_v6 else None
        if parse:
            self.parse()

    def parse(self):
        fr = gf_frames(self.n, self.frames.shape[1] if self.n else 64, _ptr(self.frames), _ptr(self.len))
        o = gf_pkt_cols_out(_ptr(self.ethertype), _ptr(self.saddr4), _ptr(self.daddr4), _ptr(self.proto),
                            _ptr(self.l4_off), _ptr(self.l4w0), _ptr(self.l4w3), _ptr(self.saddr6),
                            _ptr(self.daddr6))
        _check(lib.gf_parse_frames(C.byref(fr), C.byref(o), _stream()), "gf_parse_frames")

    def cols(self):
        return gf_pkt_cols(self.n, _ptr(self.len), _ptr(self.ethertype), _ptr(self.saddr4), _ptr(self.daddr4),
                           _ptr(self.proto), _ptr(self.l4_off), _ptr(self.l4w0), _ptr(self.l4w3),
                           _ptr(self.saddr6), _ptr(self.daddr6), _ptr(self.src_identity), _ptr(self.ifindex),
                           _ptr(self.lxc_id), _ptr(self.tc_index), _ptr(self.flow_hash))

    def columns_numpy(self):
        torch = _torch()
        torch.cuda.synchronize()
        g = lambda t, dt: t.cpu().numpy().view(dt)
        out = {"ethertype": g(self.ethertype, np.uint16), "saddr4": g(self.saddr4, np.uint32),
               "daddr4": g(self.daddr4, np.uint32), "proto": g(self.proto, np.uint8),
               "l4_off": g(self.l4_off, np.int16), "l4w0": g(self.l4w0, np.uint32), "l4w3": g(self.l4w3, np.uint16)}
        if self.saddr6 is not None:
            out["saddr6"] = self.saddr6.cpu().numpy()
            out["daddr6"] = self.daddr6.cpu().numpy()
        return out


class Datapath:
    """Installs a synth.Scenario into libgpuflow and exposes the classify calls."""

    def __init__(self, sc, pin_prefix=""):
        self.sc = sc
        self.fd = {}
        self._resp = {}
        self._tun = {}
        self._fwd = []
        self.ring = None
        for name, m in sc.maps.items():
            fd = bpf.CreateMap(m.type, m.ksz, m.vsz, m.max_entries, m.flags)
            if m.n():
                k = np.ascontiguousarray(m.keys, np.uint8)
                v = np.ascontiguousarray(m.vals, np.uint8)
                bpf.UpdateBatch(fd, k.ctypes.data, v.ctypes.data, m.n(), bpf.BPF_ANY)
            if pin_prefix is not None:
                try:
                    bpf.ObjPin(fd, bpf.MapPath(pin_prefix + name))
                except OSError:
                    pass
            self.fd[name] = fd
        h = lambda name: self.fd[name] if name else 0
        nd = sc.node or {}
        ncfg = gf_node_cfg(sc.host_ifindex, h(nd.get("proxy4")), h(nd.get("proxy6")), nd.get("ipv4_gateway", 0),
                           (C.c_uint8 * 16)(*nd.get("host_ip6", bytes(16))), (C.c_uint8 * 6)(*nd.get("host_mac", bytes(6))),
                           (C.c_uint8 * 6)(*nd.get("node_mac", bytes(6))), h(nd.get("lxc_map")),
                           nd.get("ipv4_cluster_range", 0), nd.get("ipv4_cluster_mask", 0), nd.get("ipv4_loopback", 0),
                           nd.get("ipv4_mask", 0), nd.get("encap_ifindex", 0), h(nd.get("tunnel_map")),
                           (C.c_uint8 * 16)(*nd.get("router_ip6", bytes(16))))
        _check(lib.gf_node_config(C.byref(ncfg)), "gf_node_config")
        self.xdp_prog = self.lb_prog = self.policy_array = None
        if sc.xdp:
            x = sc.xdp
            cfg = gf_xdp_cfg(h(x.get("cidr4_hmap")), h(x.get("cidr4_lmap")), h(x.get("cidr6_hmap")),
                             h(x.get("cidr6_lmap")), h(x.get("lxc_map")))
            self.xdp_prog = _check(lib.gf_xdp_prog_load(C.byref(cfg)), "gf_xdp_prog_load")
        if sc.lb:
            cfg = gf_lb_cfg(h(sc.lb.get("lb4")), h(sc.lb.get("lb6")), sc.lb["flags"], sc.lb.get("redirect_ifindex", 0))
            self.lb_prog = _check(lib.gf_lb_prog_load(C.byref(cfg)), "gf_lb_prog_load")
            if sc.lb.get("dstmac") is not None:             # LB_DSTMAC (bpf_lb.c:200-205)
                _check(lib.gf_lb_prog_set_dstmac(self.lb_prog, (C.c_uint8 * 6)(*sc.lb["dstmac"])),
                       "gf_lb_prog_set_dstmac")
        if sc.lxc:
            self.policy_array = _check(lib.gf_policy_array_create(), "gf_policy_array_create")
            self.lxc_progs = []
            for e in sc.lxc:
                cfg = gf_lxc_cfg()
                cfg.lxc_id, cfg.seclabel = e["lxc_id"], e["seclabel"]
                cfg.policy_map, cfg.ct_map4, cfg.ct_map6 = h(e.get("policy")), h(e.get("ct4")), h(e.get("ct6"))
                cfg.cidr4_ingress_map, cfg.cidr6_ingress_map = h(e.get("cidr4")), h(e.get("cidr6"))
                cfg.revnat4_map, cfg.revnat6_map = h(e.get("revnat4")), h(e.get("revnat6"))
                cfg.flags = e["flags"]
                l4 = e.get("l4") or []
                cfg.n_l4_ingress = len(l4)
                for i, (port, proxy, nh) in enumerate(l4):
                    cfg.l4_ingress[i].port = ((port & 0xff) << 8) | (port >> 8)
                    cfg.l4_ingress[i].proxy = ((proxy & 0xff) << 8) | (proxy >> 8)
                    cfg.l4_ingress[i].nexthdr = nh
                egress_fields(cfg, e, h)
                p = _check(lib.gf_lxc_prog_load(C.byref(cfg)), "gf_lxc_prog_load")
                self.lxc_progs.append(p)
                _check(lib.gf_policy_array_update(self.policy_array, e["lxc_id"], p), "gf_policy_array_update")

        self.pipe = None
        if sc.netdev and self.policy_array:
            nd = sc.netdev
            ncfg = gf_netdev_cfg(h(nd["lxc_map"]), nd.get("flags", 0), nd.get("fixed_secctx", 0),
                                 (C.c_uint8 * 16)(*nd.get("router_ip6", bytes(16))), nd.get("ingress_ifindex", 0))
            pcfg = gf_pipeline_cfg(self.xdp_prog or 0, self.lb_prog or 0, ncfg, self.policy_array)
            self.pipe = _check(lib.gf_pipeline_load(C.byref(pcfg)), "gf_pipeline_load")

        # the program on the tunnel device (bpf_overlay.c), sc.overlay = {lxc_map, flags, ingress_ifindex}
        self.ovl = None
        if getattr(sc, "overlay", None) and self.policy_array:
            ov = sc.overlay
            ocfg = gf_overlay_cfg(h(ov["lxc_map"]), ov.get("flags", 0), ov.get("ingress_ifindex", 0), self.policy_array)
            self.ovl = _check(lib.gf_overlay_load(C.byref(ocfg)), "gf_overlay_load")

        # the program on cilium_host (bpf_netdev.c with FROM_HOST), sc.host = {lxc_map, flags, fixed_secctx,
        # router_ip6, ingress_ifindex, cilium_net_mac}
        self.host = None
        if getattr(sc, "host", None) and self.policy_array:
            ho = sc.host
            ncfg = gf_netdev_cfg(h(ho["lxc_map"]), ho.get("flags", 0), ho.get("fixed_secctx", 0),
                                 (C.c_uint8 * 16)(*ho.get("router_ip6", bytes(16))), ho.get("ingress_ifindex", 0))
            hcfg = gf_host_cfg(ncfg, (C.c_uint8 * 6)(*ho.get("cilium_net_mac", bytes(6))), self.policy_array)
            self.host = _check(lib.gf_host_load(C.byref(hcfg)), "gf_host_load")

    # ---- classify calls -------------------------------------------------
    def xdp(self, b):
        torch = _torch()
        out = torch.empty(b.n, dtype=torch.uint8, device=b.device)
        c = b.cols()
        _check(lib.gf_xdp_classify(self.xdp_prog, C.byref(c), _ptr(out), _stream()), "gf_xdp_classify")
        return out

    def xdp_filter_frames(self, b, max_out=None, frames=True, verdict=True, index=True):
        """gf_xdp_filter_frames: the prefilter over the batch's frames.  Returns (verdict [n] u8,
        frames [max_out,stride] u8, len [max_out] i32, index [max_out] i32, counts [4] i32 =
        passed, dropped, written, 0), all on the device; the first counts[2] rows of frames, len
        and index are the XDP_PASS frames in batch order.  max_out: their capacity (default b.n).
        frames=False: verdict and counts only (frames, len and index are None); verdict=False /
        index=False: that output is not taken (None)."""
        torch = _torch()
        cap = b.n if max_out is None else max_out
        stride = b.frames.shape[1] if b.n else 64
        e = lambda dt, *shape: torch.empty(shape, dtype=dt, device=b.device)
        v = e(torch.uint8, b.n) if verdict else None
        snap = e(torch.uint8, cap, stride) if frames else None
        ln = e(torch.int32, cap) if frames else None
        ix = e(torch.int32, cap) if frames and index else None
        counts = e(torch.int32, 4)
        fr = gf_frames(b.n, stride, _ptr(b.frames), _ptr(b.len))
        o = gf_xdp_frames_out(_ptr(v), _ptr(snap), _ptr(ln), _ptr(ix), cap, _ptr(counts))
        _check(lib.gf_xdp_filter_frames(self.xdp_prog, C.byref(fr), C.byref(o), _stream()), "gf_xdp_filter_frames")
        return v, snap, ln, ix, counts

    def lb(self, b):
        torch = _torch()
        out = torch.empty((b.n, 12), dtype=torch.uint8, device=b.device)
        nd6 = torch.empty((b.n, 16), dtype=torch.uint8, device=b.device)
        c = b.cols()
        _check(lib.gf_lb_classify(self.lb_prog, C.byref(c), _ptr(out), _ptr(nd6), _stream()), "gf_lb_classify")
        return out, nd6

    def lb_frames(self, b, snap_out=True):
        """gf_lb_classify_frames: bpf_lb's from-netdev over the batch's frames.  snap_out: True = a
        fresh buffer, False = records only (NULL), "inplace" = b.frames itself, or a tensor of
        b.frames' shape.  Returns (records [n,12] u8, new_daddr6 [n,16] u8, frames as the program
        left them [n,stride] u8 or None)."""
        torch = _torch()
        out = torch.empty((b.n, 12), dtype=torch.uint8, device=b.device)
        nd6 = torch.empty((b.n, 16), dtype=torch.uint8, device=b.device)
        if snap_out is True:
            snap = torch.empty_like(b.frames)
        elif snap_out is False or snap_out is None:
            snap = None
        elif isinstance(snap_out, str):
            assert snap_out == "inplace"
            snap = b.frames
        else:
            snap = snap_out
        stride = b.frames.shape[1] if b.n else 64
        fr = gf_frames(b.n, stride, _ptr(b.frames), _ptr(b.len))
        _check(lib.gf_lb_classify_frames(self.lb_prog, C.byref(fr), _ptr(b.flow_hash), _ptr(out), _ptr(nd6), _ptr(snap),
                                         _stream()), "gf_lb_classify_frames")
        return out, nd6, snap

    def ingress(self, b, now, out=None):
        torch = _torch()
        if out is None:
            out = torch.empty((b.n, 8), dtype=torch.uint8, device=b.device)
        c = b.cols()
        _check(lib.gf_policy_ingress_classify(self.policy_array, C.byref(c), now, _ptr(out), _stream()),
               "gf_policy_ingress_classify")
        return out

    def ingress_batches(self, bs, nows, outs=None):
        """gf_policy_ingress_classify_batches: the batches in order, each batch's
        schedule built on a second stream while the previous one runs."""
        torch = _torch()
        if outs is None:
            outs = [torch.empty((b.n, 8), dtype=torch.uint8, device=b.device) for b in bs]
        cols = [b.cols() for b in bs]
        k = len(bs)
        cp = (C.POINTER(gf_pkt_cols) * k)(*[C.pointer(c) for c in cols])
        nw = (C.c_uint32 * k)(*[int(x) for x in nows])
        op = (C.c_void_p * k)(*[_ptr(o) for o in outs])
        _check(lib.gf_policy_ingress_classify_batches(self.policy_array, k, cp, nw, op, _stream()),
               "gf_policy_ingress_classify_batches")
        return outs

    def pipeline(self, b, now, out=None, snap_out=True):
        """Full pipeline over the batch's frames: returns (records [n,24] u8,
        new_daddr6 [n,16] u8, rewritten snaps [n,stride] u8 or None)."""
        torch = _torch()
        if out is None:
            out = torch.empty((b.n, 24), dtype=torch.uint8, device=b.device)
        nd6 = torch.empty((b.n, 16), dtype=torch.uint8, device=b.device)
        snap = torch.empty_like(b.frames) if snap_out else None
        stride = b.frames.shape[1] if b.n else 64
        pb = gf_pipe_batch(gf_frames(b.n, stride, _ptr(b.frames), _ptr(b.len)), _ptr(b.tc_index), _ptr(b.flow_hash))
        _check(lib.gf_pipeline_classify(self.pipe, C.byref(pb), now, _ptr(out), _ptr(nd6), _ptr(snap), _stream()),
               "gf_pipeline_classify")
        return out, nd6, snap

    def pipeline_tunnel(self, b, now, out=None, snap_out=True, tunnel_ip=True):
        """gf_pipeline_classify_tunnel: pipeline() with the tunnel endpoint column of a netdev stage
        loaded with GF_NETDEV_F_ENCAP.  Returns (records, new_daddr6, rewritten snaps or None,
        tunnel_ip [n] i32 — bpf_tunnel_key.remote_ipv4, 0 where the frame did not encap — or None
        when tunnel_ip=False, which passes NULL)."""
        torch = _torch()
        if out is None:
            out = torch.empty((b.n, 24), dtype=torch.uint8, device=b.device)
        nd6 = torch.empty((b.n, 16), dtype=torch.uint8, device=b.device)
        snap = torch.empty_like(b.frames) if snap_out else None
        tun = torch.empty(b.n, dtype=torch.int32, device=b.device) if tunnel_ip else None
        stride = b.frames.shape[1] if b.n else 64
        pb = gf_pipe_batch(gf_frames(b.n, stride, _ptr(b.frames), _ptr(b.len)), _ptr(b.tc_index), _ptr(b.flow_hash))
        _check(lib.gf_pipeline_classify_tunnel(self.pipe, C.byref(pb), now, _ptr(out), _ptr(nd6), _ptr(snap), _ptr(tun),
                                               _stream()), "gf_pipeline_classify_tunnel")
        return out, nd6, snap, tun

    def overlay(self, b, now, out=None, snap_out=True, opt=None, opt_len=None):
        """from-overlay over the batch's inner frames and tunnel ids (+ handle_policy of
        the local deliveries): returns (records [n,24] u8, rewritten snaps or None).
        opt [n,opt_stride] u8 / opt_len [n] u8 (device tensors): the packets' tunnel options, for
        a program loaded with GF_OVERLAY_F_GENEVE (gf_overlay_classify_opts); given either of
        them the call goes there, with neither to gf_overlay_classify."""
        torch = _torch()
        if out is None:
            out = torch.empty((b.n, 24), dtype=torch.uint8, device=b.device)
        snap = torch.empty_like(b.frames) if snap_out else None
        stride = b.frames.shape[1] if b.n else 64
        ob = gf_overlay_batch(gf_frames(b.n, stride, _ptr(b.frames), _ptr(b.len)), _ptr(b.tunnel_id), _ptr(b.tc_index),
                              _ptr(b.flow_hash))
        if opt is None and opt_len is None:
            _check(lib.gf_overlay_classify(self.ovl, C.byref(ob), now, _ptr(out), _ptr(snap), _stream()),
                   "gf_overlay_classify")
        else:
            to = gf_tunnel_opts(_ptr(opt), opt.shape[1] if opt is not None and opt.dim() == 2 else 0, _ptr(opt_len))
            _check(lib.gf_overlay_classify_opts(self.ovl, C.byref(ob), C.byref(to), now, _ptr(out), _ptr(snap),
                                                _stream()), "gf_overlay_classify_opts")
        return out, snap

    def egress_tunnel_meta(self, lxc_id, records):
        """gf_lxc_egress_tunnel_meta: what encap_and_redirect sets besides the record's tunnel_ip for
        the GF_EG_F_ENCAP records of egress() — lxc_id [n] i16 the batch's column, records [n,24] u8.
        Returns (tunnel_id [n] i32, opt [n,8] u8, opt_len [n] u8): the sender's SECLABEL, its
        GENEVE_OPTS and 8; zeros for every other record.  The layout overlay() takes."""
        torch = _torch()
        n = records.shape[0]
        tid = torch.empty(n, dtype=torch.int32, device=records.device)
        opt = torch.empty((n, 8), dtype=torch.uint8, device=records.device)
        ol = torch.empty(n, dtype=torch.uint8, device=records.device)
        _check(lib.gf_lxc_egress_tunnel_meta(self.policy_array, _ptr(lxc_id), _ptr(records), n, _ptr(tid), _ptr(opt),
                                             _ptr(ol), _stream()), "gf_lxc_egress_tunnel_meta")
        return tid, opt, ol

    def from_host(self, b, now, out=None, snap_out=True):
        """from-host (cilium_host) over the batch's frames and marks (+ handle_policy of the
        local deliveries): returns (records [n,24] u8, rewritten snaps or None)."""
        torch = _torch()
        if out is None:
            out = torch.empty((b.n, 24), dtype=torch.uint8, device=b.device)
        snap = torch.empty_like(b.frames) if snap_out else None
        stride = b.frames.shape[1] if b.n else 64
        hb = gf_host_batch(gf_frames(b.n, stride, _ptr(b.frames), _ptr(b.len)), _ptr(b.mark), _ptr(b.tc_index),
                           _ptr(b.flow_hash))
        _check(lib.gf_host_classify(self.host, C.byref(hb), now, _ptr(out), _ptr(snap), _stream()),
               "gf_host_classify")
        return out, snap

    def egress(self, b, now, out=None, snap_out=True):
        """The from-container program over the batch's frames (+ handle_policy of the
        local deliveries): returns (records [n,24] u8, rewritten snaps or None)."""
        torch = _torch()
        if out is None:
            out = torch.empty((b.n, 24), dtype=torch.uint8, device=b.device)
        snap = torch.empty_like(b.frames) if snap_out else None
        stride = b.frames.shape[1] if b.n else 64
        eb = gf_lxc_batch(gf_frames(b.n, stride, _ptr(b.frames), _ptr(b.len)), _ptr(b.lxc_id), _ptr(b.flow_hash))
        _check(lib.gf_lxc_egress_classify(self.policy_array, C.byref(eb), now, _ptr(out), _ptr(snap), _stream()),
               "gf_lxc_egress_classify")
        return out, snap

    # ---- ARP / ICMPv6 responders (the tail calls after a classify call) ----
    def responder(self, flags=0, max_len=0):
        """The gf_respond handle over this datapath's cilium_policy array (loaded on first use,
        one per (flags, max_len))."""
        key = (flags, max_len)
        if key not in self._resp:
            cfg = gf_respond_cfg(self.policy_array or 0, flags, max_len)
            self._resp[key] = _check(lib.gf_respond_load(C.byref(cfg)), "gf_respond_load")
        return self._resp[key]

    def respond(self, frames, len, call, lxc_id=None, flow_hash=None, snap_out=None, flags=0, max_len=0):
        """gf_respond over frames [n,stride] u8, len [n] i32, call [n] u8 (device tensors); lxc_id
        [n] i16: the endpoints whose objects make the calls, None = the node's programs.  Returns
        (records [n,8] u8, snap_out [n,stride] u8); rows of frames without a call keep what snap_out
        held (a fresh buffer: uninitialised)."""
        torch = _torch()
        n = frames.shape[0]
        out = torch.empty((n, 8), dtype=torch.uint8, device=frames.device)
        if snap_out is None:
            snap_out = torch.empty_like(frames)
        rb = gf_respond_batch(gf_frames(n, frames.shape[1], _ptr(frames), _ptr(len)), _ptr(call), _ptr(lxc_id),
                              _ptr(flow_hash))
        _check(lib.gf_respond(self.responder(flags, max_len), C.byref(rb), _ptr(out), _ptr(snap_out), _stream()),
               "gf_respond")
        return out, snap_out

    def respond_calls(self, kind, frames, len, records):
        """gf_respond_calls: the GF_CALL_* column of a classify call's records (kind GF_REC_*)."""
        torch = _torch()
        n = frames.shape[0]
        call = torch.empty(n, dtype=torch.uint8, device=frames.device)
        fr = gf_frames(n, frames.shape[1], _ptr(frames), _ptr(len))
        _check(lib.gf_respond_calls(C.byref(fr), _ptr(records), kind, _ptr(call), _stream()), "gf_respond_calls")
        return call

    def respond_after(self, kind, b, records, snap, flags=0, max_len=0):
        """The responder tail calls of a classified batch: kind GF_REC_EGRESS (records of
        egress()) or GF_REC_PIPELINE (pipeline(), overlay(), from_host()), b the DeviceBatch,
        snap the entry point's snap_out.  ARP, NS and echo frames are taken as received
        (b.frames; the pipeline's GF_PIPE_F_RESPONDER records of a netdev stage with
        GF_NETDEV_F_HANDLE_NS included: their call comes from the record, and bpf_lb leaves an
        ICMPv6 frame that matches no service as it came); time-exceeded frames as the entry point
        left them (snap): ipv6_l3 returns
        before its first write, the programs in front of it (LB, reverse proxy, dmac rewrite)
        do not.  Egress batches pass the sender's lxc_id, the others the node's NODE_MAC.
        Returns (call [n] u8, records [n,8] u8, reply frames [n,stride] u8)."""
        torch = _torch()
        call = self.respond_calls(kind, b.frames, b.len, records)
        te = (call == GF_CALL_ICMP6_TIME_EXCEEDED).unsqueeze(1)
        frames = torch.where(te, snap, b.frames)
        out, reply = self.respond(frames, b.len, call, b.lxc_id if kind == GF_REC_EGRESS else None, b.flow_hash,
                                  flags=flags, max_len=max_len)
        return call, out, reply

    # ---- VXLAN / Geneve on the wire (the kernel's tunnel device in the reference) ----
    def tunnel_load(self, mode, dst_port, local_ip=0, flags=0, sport_min=32768, sport_max=61000, ttl=64, tos=0,
                    src_mac=bytes(6), dst_mac=bytes(6)):
        """gf_tunnel_load: a tunnel endpoint handle (closed with the datapath).  Addresses as
        gf_egress_out.tunnel_ip (10.0.0.1 = 0x0a000001); dst_port has no default."""
        cfg = gf_tunnel_cfg(mode, flags, local_ip & 0xFFFFFFFF, dst_port, sport_min, sport_max, ttl, tos,
                            (C.c_uint8 * 6)(*src_mac), (C.c_uint8 * 6)(*dst_mac))
        h = _check(lib.gf_tunnel_load(C.byref(cfg)), "gf_tunnel_load")
        self._tun[h] = mode
        return h

    def tunnel_select(self, kind, records):
        """gf_tunnel_select: the select column of tunnel_encap from a classify call's records
        (kind GF_REC_EGRESS: GF_EG_F_ENCAP; GF_REC_PIPELINE: the redirect to ENCAP_IFINDEX)."""
        torch = _torch()
        n = records.shape[0]
        sel = torch.empty(n, dtype=torch.uint8, device=records.device)
        _check(lib.gf_tunnel_select(_ptr(records), kind, n, _ptr(sel), _stream()), "gf_tunnel_select")
        return sel

    def tunnel_encap(self, tun, frames, len, remote_ip, tunnel_id, out_stride, opt=None, opt_len=None, select=None,
                     flow_hash=None, ip_id=None, dst_mac=None, out=None):
        """gf_tunnel_encap over inner frames [n,stride] u8, len / remote_ip / tunnel_id [n] i32 and the
        optional columns (device tensors; opt [n,opt_stride] u8, ip_id [n] i16, dst_mac [n,6] u8).
        Returns (out [n,out_stride] u8, out_len [n] i32, status [n] u8); rows of frames that are not
        GF_TUN_ST_OK keep what `out` held (a fresh buffer: uninitialised)."""
        torch = _torch()
        n = frames.shape[0]
        if out is None:
            out = torch.empty((n, out_stride), dtype=torch.uint8, device=frames.device)
        out_len = torch.empty(n, dtype=torch.int32, device=frames.device)
        status = torch.empty(n, dtype=torch.uint8, device=frames.device)
        tx = gf_tunnel_tx(gf_frames(n, frames.shape[1], _ptr(frames), _ptr(len)), _ptr(remote_ip), _ptr(tunnel_id),
                          _ptr(opt), opt.shape[1] if opt is not None else 0, _ptr(opt_len), _ptr(select),
                          _ptr(flow_hash), _ptr(ip_id), _ptr(dst_mac))
        _check(lib.gf_tunnel_encap(tun, C.byref(tx), _ptr(out), out_stride, _ptr(out_len), _ptr(status), _stream()),
               "gf_tunnel_encap")
        return out, out_len, status

    def tunnel_decap(self, tun, outer, len, inner_stride=128, opt_stride=8):
        """gf_tunnel_decap over outer frames [n,stride] u8 and len [n] i32.  Returns a namespace in
        the layout overlay() takes: frames [n,inner_stride] u8, len, tunnel_id, outer_saddr [n] i32,
        opt [n,opt_stride] u8 (zeros; written in Geneve mode), opt_len, status [n] u8, plus n, device,
        tc_index and flow_hash None.  Rows and columns of frames that are not OK keep the zeros the
        buffers start with (len is written for every frame)."""
        import types
        torch = _torch()
        n, dev = outer.shape[0], outer.device
        z = lambda dt, *shape: torch.zeros((n,) + shape, dtype=dt, device=dev)
        r = types.SimpleNamespace(n=n, device=dev, frames=z(torch.uint8, inner_stride), len=z(torch.int32),
                                  tunnel_id=z(torch.int32), outer_saddr=z(torch.int32), opt=z(torch.uint8, opt_stride),
                                  opt_len=z(torch.uint8), status=z(torch.uint8), tc_index=None, flow_hash=None)
        fr = gf_frames(n, outer.shape[1], _ptr(outer), _ptr(len))
        ro = gf_tunnel_rx_out(_ptr(r.frames), inner_stride, _ptr(r.len), _ptr(r.tunnel_id), _ptr(r.outer_saddr),
                              _ptr(r.opt), opt_stride, _ptr(r.opt_len), _ptr(r.status))
        _check(lib.gf_tunnel_decap(tun, C.byref(fr), C.byref(ro), _stream()), "gf_tunnel_decap")
        return r

    # ---- forwarding the verdicts: the frames of a classified batch, packed per output queue ----
    def forward_load(self, n_queues, stack_queue=GF_FWD_DROP, responder_queue=GF_FWD_DROP, default_queue=GF_FWD_DROP,
                     ifindex=()):
        """gf_forward_load: a forward handle (closed with the datapath).  ifindex: (ifindex_lo, queue)
        pairs, a later pair for the same ifindex_lo winning; a queue is < n_queues or GF_FWD_DROP."""
        ent = (gf_forward_ifindex * max(len(ifindex), 1))(*[gf_forward_ifindex(i, q, 0) for i, q in ifindex])
        cfg = gf_forward_cfg(n_queues, stack_queue, responder_queue, default_queue, 0, len(ifindex),
                             ent if len(ifindex) else None)
        h = _check(lib.gf_forward_load(C.byref(cfg)), "gf_forward_load")
        self._fwd.append(h)
        return h

    def forward_queues(self, fwd, kind, records):
        """gf_forward_queues: the queue column [n] u8 of a classify call's records (kind GF_REC_EGRESS,
        GF_REC_PIPELINE or GF_REC_LB), by the rule table of include/gpuflow.h."""
        torch = _torch()
        n = records.shape[0]
        queue = torch.empty(n, dtype=torch.uint8, device=records.device)
        _check(lib.gf_forward_queues(fwd, _ptr(records), kind, n, _ptr(queue), _stream()), "gf_forward_queues")
        return queue

    def forward_frames(self, frames, len, queue, n_queues, max_out=None, index=True):
        """gf_forward_frames over frames [n,stride] u8, len [n] i32 and a queue column [n] u8 (device
        tensors).  Returns (frames [max_out,stride] u8, len [max_out] i32, index [max_out] i32 or
        None, qoff [n_queues + 1] i32, counts [4] i32 = forwarded, not forwarded, written, invalid
        queue bytes), all on the device: queue q owns rows [qoff[q], qoff[q + 1]), in arrival
        order; the first counts[2] rows are defined.  max_out: the capacity in rows (default n)."""
        torch = _torch()
        n = frames.shape[0]
        cap = n if max_out is None else max_out
        e = lambda dt, *shape: torch.empty(shape, dtype=dt, device=frames.device)
        snap, ln = e(torch.uint8, cap, frames.shape[1]), e(torch.int32, cap)
        ix = e(torch.int32, cap) if index else None
        qoff, counts = e(torch.int32, n_queues + 1), e(torch.int32, 4)
        fr = gf_frames(n, frames.shape[1], _ptr(frames), _ptr(len))
        o = gf_forward_out(_ptr(snap), _ptr(ln), _ptr(ix), cap, _ptr(qoff), _ptr(counts))
        _check(lib.gf_forward_frames(C.byref(fr), _ptr(queue), n_queues, C.byref(o), _stream()), "gf_forward_frames")
        return snap, ln, ix, qoff, counts

    # ---- the event ring and its drain (cilium monitor's filters on the device) ----
    def set_event_ring(self, capacity, device="cuda"):
        """gf_set_event_ring over a fresh ring of `capacity` slots (None: no ring).  The ring is
        the library's, not this object's: close() unsets it."""
        torch = _torch()
        if capacity is None:
            _check(lib.gf_set_event_ring(None), "gf_set_event_ring")
            self.ring = None
            return None
        recs = torch.zeros((max(capacity, 1), GF_EVENT_RECORD), dtype=torch.uint8, device=device)
        cnt = torch.zeros(1, dtype=torch.int32, device=device)
        self.ring = (recs, cnt, gf_event_ring(recs.data_ptr(), capacity, cnt.data_ptr()))
        _check(lib.gf_set_event_ring(C.byref(self.ring[2])), "gf_set_event_ring")
        return self.ring

    def event_drain(self, filter, first=0, max_n=0, packed=False, reset=False, out_records=None):
        """gf_event_drain over the ring of set_event_ring with a monitor.EventFilter, on the
        current stream.  out_records: a uint8 device tensor to store into (default: room for every
        record of the window).  Returns (out, offsets, res): the output tensor, the [window + 1]
        int32 offsets tensor and the gf_event_drain_out fields as a dict (read after a stream
        synchronise; res["written"] records, res["bytes"] bytes of `out` and res["written"] + 1
        offsets are defined)."""
        torch = _torch()
        recs, cnt, ring = self.ring
        window = min(max_n or GF_EVD_MAX_WINDOW, ring.capacity)
        if out_records is None:
            out_records = torch.empty((max(min(window, max(ring.capacity - first, 0)), 1), GF_EVENT_RECORD),
                                      dtype=torch.uint8, device=recs.device)
        off = torch.empty(window + 1, dtype=torch.int32, device=recs.device)
        res = torch.zeros(C.sizeof(gf_event_drain_out), dtype=torch.uint8, device=recs.device)
        flags = (GF_EVD_F_PACKED if packed else 0) | (GF_EVD_F_RESET if reset else 0)
        _check(lib.gf_event_drain(filter.handle, C.byref(ring), first, max_n, flags, _ptr(out_records),
                                  out_records.numel(), _ptr(off), _ptr(res), _stream()), "gf_event_drain")
        torch.cuda.current_stream().synchronize()
        r = gf_event_drain_out.from_buffer_copy(res.cpu().numpy().tobytes())
        d = {k: getattr(r, k) for k, _ in gf_event_drain_out._fields_ if k != "pad"}
        d["by_type"] = list(r.by_type)
        return out_records, off, d

    # ---- proxy map sweeps (pkg/maps/proxymap: GC / Flush, CleanupOnRedirectClose) ----
    def proxy_gc(self, name, filter_time):
        """gf_proxy_gc on the current stream: deletes lifetime < filter_time, returns the count."""
        return _check(lib.gf_proxy_gc(self.fd[name], filter_time & 0xFFFFFFFF, _stream()), "gf_proxy_gc")

    def proxy_cleanup_port(self, name, port):
        """gf_proxy_cleanup_port on the current stream: deletes the TCP entries whose dport is
        `port` (host order here, stored in network order), returns the count."""
        return _check(lib.gf_proxy_cleanup_port(self.fd[name], _be16(port), _stream()), "gf_proxy_cleanup_port")

    # ---- conntrack GC (pkg/endpointmanager/conntrack.go: EnableConntrackGC) ----
    def ct_gc_round(self, now_sec):
        """One GC round on the current stream: every CT map the scenario's programs bind
        (per-endpoint and shared ones, IPv4 and IPv6), each once, in one gf_ct_gc_maps
        call.  Returns {map name: entries deleted}."""
        names = []
        for e in self.sc.lxc or []:
            for fam in ("ct4", "ct6"):
                if e.get(fam) and e[fam] not in names:
                    names.append(e[fam])
        return dict(zip(names, ctmap.GCMaps([self.fd[n] for n in names], now_sec, _stream())))

    # ---- map readback ----------------------------------------------------
    def dump_map(self, name):
        m = self.sc.maps[name]
        d = {}
        bpf_map = bpf.Map(name, m.type, m.ksz, m.vsz, m.max_entries, m.flags)
        bpf_map.fd = self.fd[name]
        bpf_map.DumpWithCallback(lambda k, v: d.__setitem__(k, v))
        return d

    def close(self):
        """Close the program objects, then the maps (a program holds its maps, so
        their device tables are released once both are closed)."""
        progs = list(self._resp.values()) + list(self._tun) + list(self._fwd) + [self.host, self.ovl, self.pipe, self.policy_array, self.lb_prog, self.xdp_prog] + list(getattr(self, "lxc_progs", []))
        for h in [h for h in progs if h] + list(self.fd.values()):
            try:
                bpf.ObjClose(h)
            except OSError:
                pass
        self.host = self.ovl = self.pipe = self.policy_array = self.lb_prog = self.xdp_prog = None
        self.lxc_progs = []
        self._resp = {}
        self._tun = {}
        self._fwd = []
        self.fd = {}
        if getattr(self, "ring", None) is not None:
            self.set_event_ring(None)


def to_numpy(t, dtype):
    return t.cpu().numpy().view(dtype).reshape(-1)
