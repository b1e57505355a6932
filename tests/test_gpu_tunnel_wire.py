"""gf_tunnel_encap / gf_tunnel_decap (k_tun_encap, k_tun_decap) on the GPU: the field-by-field KATs,
fuzz batches bit for bit against tests/tunnel_model.py (rows with their poison, out_len, status and
every receive column), batch sizes around the wave and the tile, the device round trip, and the
chain from node A's from-container program to node B's from-overlay program."""
import ctypes as C
import errno
import types

import numpy as np
import pytest

from cilium_amd import synth
from tests import tunnel_model as TM
from tests.test_tunnel_wire import KATS, FUZZ_CFG, kat_cfg, kat_frame

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

POISON = TM.POISON
P32 = np.uint32(POISON * 0x01010101)
SIGNED = {np.dtype(np.uint32): np.int32, np.dtype(np.uint16): np.int16, np.dtype(np.uint8): np.uint8}


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(0)


def _dev(a, dt=np.uint8):
    if a is None:
        return None
    a = np.ascontiguousarray(np.asarray(a).astype(dt, copy=False))
    return torch.from_numpy(a.view(SIGNED[np.dtype(dt)])).cuda()


def _np(t, dt=np.uint8):
    return t.cpu().numpy().view(dt)


@pytest.fixture(scope="module")
def dp():
    _gpu()
    from cilium_amd.datapath import Datapath
    sc = synth.Scenario("tunnel_wire")
    sc.node = {"encap_ifindex": 7}
    d = Datapath(sc, pin_prefix=None)
    yield d
    d.close()


def _load(dp, c):
    return dp.tunnel_load(c.mode, c.dst_port, c.local_ip, c.flags, c.sport_min, c.sport_max, c.ttl, c.tos, c.src_mac, c.dst_mac)


def _encap(dp, tun, frames, lens, remote_ip, tunnel_id, out_stride, opt=None, opt_len=None, select=None, flow_hash=None,
           ip_id=None, dst_mac=None):
    """The device call over numpy columns, the output row buffer starting as poison.  Returns the
    device tensors (out, out_len, status)."""
    out = torch.full((len(lens), out_stride), POISON, dtype=torch.uint8, device="cuda")
    return dp.tunnel_encap(tun, _dev(frames), _dev(lens, np.uint32), _dev(remote_ip, np.uint32), _dev(tunnel_id, np.uint32),
                           out_stride, _dev(opt), _dev(opt_len), _dev(select), _dev(flow_hash, np.uint32),
                           _dev(ip_id, np.uint16), _dev(dst_mac), out=out)


def _decap(dp, tun, outer, lens, inner_stride, opt_stride=8, geneve=True):
    """The device call, every output starting as poison.  Returns a namespace of numpy columns."""
    from cilium_amd._lib import lib, gf_frames, gf_tunnel_rx_out
    n = outer.shape[0]
    f = lambda *shape: torch.full((n,) + shape, POISON, dtype=torch.uint8, device="cuda")
    inner, il, tid, sa, opt, ol, st = f(inner_stride), f(4), f(4), f(4), f(opt_stride), f(), f()
    fr = gf_frames(n, outer.shape[1], outer.data_ptr(), lens.data_ptr())
    ro = gf_tunnel_rx_out(inner.data_ptr(), inner_stride, il.data_ptr(), tid.data_ptr(), sa.data_ptr(), opt.data_ptr(),
                          opt_stride, ol.data_ptr(), st.data_ptr())
    rc = lib.gf_tunnel_decap(tun, C.byref(fr), C.byref(ro), None)
    assert rc == 0, rc
    torch.cuda.synchronize()
    u32 = lambda t: t.cpu().numpy().view(np.uint32).reshape(-1)
    return types.SimpleNamespace(inner=_np(inner), inner_len=u32(il), tunnel_id=u32(tid), outer_saddr=u32(sa), opt=_np(opt),
                                 opt_len=_np(ol), status=_np(st))


def _same_rows(got, want, what):
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert not len(bad), (what, len(bad), int(bad[0]), np.nonzero(got[bad[0]] != want[bad[0]])[0][:8])


def _same_col(got, want, what):
    bad = np.nonzero(got != want)[0]
    assert not len(bad), (what, len(bad), int(bad[0]), got[bad[0]], want[bad[0]])


def _same_rx(got, want, what):
    _same_col(got.status, want.status, what + " status")
    _same_col(got.inner_len, want.inner_len, what + " inner_len")
    _same_rows(got.inner, want.inner, what + " inner rows")
    _same_col(got.tunnel_id, want.tunnel_id, what + " tunnel_id")
    _same_col(got.outer_saddr, want.outer_saddr, what + " outer_saddr")
    _same_col(got.opt_len, want.opt_len, what + " opt_len")
    _same_rows(got.opt, want.opt, what + " opt rows")


# ---------------------------------------------------------------- KATs
def test_gpu_kats_encap(dp):
    for e in KATS["encap"]:
        c = kat_cfg(e["cfg"])
        tun = _load(dp, c)
        S = e["snap_stride"]
        fr = np.frombuffer(bytes.fromhex(e["frame"]), np.uint8).reshape(1, S)
        os_ = e["opt_stride"]
        opt = np.frombuffer(bytes.fromhex(e["opt"]), np.uint8).reshape(1, os_) if os_ else None
        out, ol, st = _encap(dp, tun, fr, [e["len"]], [e["remote_ip"]], [e["tunnel_id"]], e["out_stride"], opt,
                             [e["opt_len"]] if os_ else None, [e["select"]], [e["flow_hash"]], [e["ip_id"]],
                             np.frombuffer(bytes.fromhex(e["dst_mac"]), np.uint8).reshape(1, 6) if e["dst_mac"] else None)
        torch.cuda.synchronize()
        want = np.full(e["out_stride"], POISON, np.uint8)
        if e["outer"] is not None:
            w = kat_frame(e["outer"])[:e["out_stride"]]
            want[:len(w)] = np.frombuffer(w, np.uint8)
        assert (int(_np(st)[0]), int(_np(ol, np.uint32)[0])) == (e["status"], e["out_len"]), e["name"]
        assert np.array_equal(_np(out)[0], want), (e["name"], np.nonzero(_np(out)[0] != want)[0][:8])


def test_gpu_kats_decap(dp):
    for d in KATS["decap"]:
        c = kat_cfg(d["cfg"])
        tun = _load(dp, c)
        S = d["snap_stride"]
        fr = kat_frame(d["outer"], d.get("cut"))[:S].ljust(S, b"\0")
        got = _decap(dp, tun, _dev(np.frombuffer(fr, np.uint8).reshape(1, S)), _dev([d["len"]], np.uint32), d["inner_stride"],
                     d["opt_stride"])
        w = d["want"]
        assert (int(got.status[0]), int(got.inner_len[0])) == (w["status"], w["inner_len"]), d["name"]
        inner, opt = np.full(d["inner_stride"], POISON, np.uint8), np.full(d["opt_stride"], POISON, np.uint8)
        tid = sa = int(P32)
        ol = POISON
        if w["status"] in (TM.ST_OK, TM.ST_OK_UNVERIFIED):
            b = bytes.fromhex(w["inner"])
            inner[:len(b)] = np.frombuffer(b, np.uint8)
            b = bytes.fromhex(w["opt"])
            opt[:len(b)] = np.frombuffer(b, np.uint8)
            tid, sa, ol = w["tunnel_id"], w["outer_saddr"], w["opt_len"]
        assert np.array_equal(got.inner[0], inner) and np.array_equal(got.opt[0], opt), d["name"]
        assert (int(got.tunnel_id[0]), int(got.outer_saddr[0]), int(got.opt_len[0])) == (tid, sa, ol), d["name"]


# ---------------------------------------------------------------- fuzz, round trip, receive negatives
NEG_RX = 24     # outer frames damaged per receive status


def _damage(rng, outer, out_len, ok, mode, csum):
    """NEG_RX frames each: another ethertype (NOT_TUNNEL), a header checksum bit (BAD_OUTER), the
    tunnel header's first byte (BAD_HDR) and, with a checksum, a bit of the first inner byte
    (BAD_CSUM; inside every snap).  Returns the rows chosen per kind."""
    cand = rng.permutation(np.nonzero(ok & (out_len <= outer.shape[1]))[0])
    picks = [cand[k * NEG_RX:(k + 1) * NEG_RX] for k in range(4)]
    outer[picks[0], 12] = 0x86
    outer[picks[1], 24] ^= 0x10
    outer[picks[2], 42] ^= 0xC0 if mode else 0x08
    if csum:
        outer[picks[3], 50 + 4] ^= 0x01
    return picks


@pytest.mark.parametrize("mode", [0, 1], ids=["vxlan", "geneve"])
@pytest.mark.parametrize("csum", [0, 1], ids=["nocsum", "csum"])
@pytest.mark.parametrize("S,OS", [(64, 128), (122, 320), (128, 512), (256, 320)])
def test_gpu_fuzz_encap_decap(dp, mode, csum, S, OS):
    """20,000 frames: encap with and without the optional columns, then decap of the device's own
    output (damaged in places), every row, column and status against the model, poison included."""
    n = 20000
    z = synth.tunnel_fuzz(n, mode, seed=100 * S + OS + 2 * mode + csum, stride=S, opt_stride=64)
    flags = (TM.F_UDP_CSUM if csum else 0) | (TM.F_DF if (S + mode) & 1 == 0 else 0)
    c = TM.cfg(mode, flags=flags, **FUZZ_CFG[mode])
    tun = _load(dp, c)
    for full in (True, False):
        kw = dict(opt=z.opt, opt_len=z.opt_len, select=z.select, flow_hash=z.flow_hash, ip_id=z.ip_id, dst_mac=z.dst_mac) \
            if full else (dict(opt=z.opt, opt_len=z.opt_len) if mode and S != 64 else {})
        out, ol, st = _encap(dp, tun, z.frames, z.lens, z.remote_ip, z.tunnel_id, OS, **kw)
        torch.cuda.synchronize()
        w_out, w_ol, w_st = TM.encap_batch(c, z.frames, z.lens, z.remote_ip, z.tunnel_id, OS, **kw)
        what = f"encap {'all' if full else 'no'} columns"
        _same_col(_np(st), w_st, what + " status")
        _same_col(_np(ol, np.uint32).reshape(-1), w_ol, what + " out_len")
        _same_rows(_np(out), w_out, what + " rows")
        if full:
            neg = z.neg
            cnt = lambda s: int((w_st == s).sum())
            assert (cnt(TM.ST_SKIPPED), cnt(TM.ST_SHORT), cnt(TM.ST_BAD_OPT)) == (neg["skipped"], neg["short"], neg["bad_opt"])
            assert cnt(TM.ST_TRUNCATED) == (neg["truncated"] if csum else 0)
            assert cnt(TM.ST_OK) == n - neg["skipped"] - neg["short"] - neg["bad_opt"] - (neg["truncated"] if csum else 0)
            keep = (out, ol, w_out.copy(), w_ol, w_st)
    # receive: the device's rows (== the model's), some damaged; local_ip 0 = any destination
    out, ol, w_out, w_ol, w_st = keep
    rng = np.random.default_rng(S + OS)
    ok = w_st == TM.ST_OK
    picks = _damage(rng, w_out, w_ol, ok, mode, csum)
    rxc = TM.cfg(mode, **{**FUZZ_CFG[mode], "local_ip": 0})
    rtun = _load(dp, rxc)
    got = _decap(dp, rtun, _dev(w_out), ol, S, 64)
    want = TM.decap_batch(rxc, w_out, w_ol, S, 64)
    _same_rx(got, want, "decap")
    for k, s in enumerate((TM.ST_NOT_TUNNEL, TM.ST_BAD_OUTER, TM.ST_BAD_HDR) + ((TM.ST_BAD_CSUM,) if csum else ())):
        assert (want.status[picks[k]] == s).all() and len(picks[k]) == NEG_RX, s
    # the round trip of every undamaged frame: x, its columns and len come back
    hit = np.zeros(n, bool)
    hit[np.concatenate(picks[:4 if csum else 3])] = True
    rt = ok & ~hit
    assert rt.sum() >= n - 4 * 16 - 4 * NEG_RX
    assert np.isin(got.status[rt], (TM.ST_OK, TM.ST_OK_UNVERIFIED)).all()
    assert ((got.status[rt] == TM.ST_OK_UNVERIFIED) == (csum == 1) & (w_ol[rt] > OS)).all()
    _same_col(got.inner_len[rt], z.lens[rt], "round trip len")
    _same_col(got.tunnel_id[rt], z.tunnel_id[rt] & 0xffffff, "round trip tunnel_id")
    assert (got.outer_saddr[rt] == c.local_ip).all()
    olw = z.opt_len[rt] if mode else np.zeros(rt.sum(), np.uint8)
    _same_col(got.opt_len[rt], olw, "round trip opt_len")
    col = np.arange(S)[None, :]
    carried = np.minimum(np.minimum(z.lens[rt], S), np.maximum(OS - 50 - olw.astype(np.int64), 0))[:, None]
    assert not ((got.inner[rt] != z.frames[rt]) & (col < carried)).any(), "round trip inner bytes"
    if mode:
        oc = np.arange(64)[None, :] < olw[:, None]
        assert not ((got.opt[rt] != z.opt[rt]) & oc).any(), "round trip options"


@pytest.mark.parametrize("mode", [0, 1], ids=["vxlan", "geneve"])
@pytest.mark.parametrize("OS,shift", [(250, 0), (203, 0), (256, 4)], ids=["stride250", "stride203", "base+4"])
def test_gpu_decap_byte_staging(dp, mode, OS, shift):
    """k_tun_decap stages rows by bytes when the outer snap_stride is no multiple of 16 or the
    buffer is not 16-byte aligned: outer frames re-laid at such strides and bases (cut where the
    stride is shorter than the frame), some damaged, every column against the model."""
    n, S = 3000, 128
    z = synth.tunnel_fuzz(n, mode, seed=7 + OS + shift, stride=S, opt_stride=64)
    c = TM.cfg(mode, flags=TM.F_UDP_CSUM, **FUZZ_CFG[mode])
    w_out, w_ol, w_st = TM.encap_batch(c, z.frames, z.lens, z.remote_ip, z.tunnel_id, 320, z.opt, z.opt_len, z.select,
                                       z.flow_hash, z.ip_id, z.dst_mac)
    outer = np.ascontiguousarray(w_out[:, :OS])
    picks = _damage(np.random.default_rng(OS), outer, w_ol, w_st == TM.ST_OK, mode, 1)
    rxc = TM.cfg(mode, **{**FUZZ_CFG[mode], "local_ip": 0})
    buf = torch.zeros(n * OS + 16, dtype=torch.uint8, device="cuda")
    dev = buf[shift:shift + n * OS].view(n, OS)
    dev.copy_(torch.from_numpy(outer))
    assert OS % 16 or dev.data_ptr() % 16
    got = _decap(dp, _load(dp, rxc), dev, _dev(w_ol, np.uint32), S, 64)
    want = TM.decap_batch(rxc, outer, w_ol, S, 64)
    _same_rx(got, want, "decap")
    for k, s in enumerate((TM.ST_NOT_TUNNEL, TM.ST_BAD_OUTER, TM.ST_BAD_HDR, TM.ST_BAD_CSUM)):
        assert (want.status[picks[k]] == s).all() and len(picks[k]) == NEG_RX, s
    assert (want.status == TM.ST_OK).sum() >= n // 2
    if mode and OS < 250:                               # 50 + 64 + 128 bytes do not fit a 203-byte snap
        assert (want.status == TM.ST_OK_UNVERIFIED).sum() >= 16


# ---------------------------------------------------------------- batch sizes
@pytest.mark.parametrize("S", [128, 256], ids=["tile128", "tile64"])
def test_gpu_batch_sizes(dp, S):
    """n around the wave (64), the block (256) and the tile (128 rows up to 128-byte snaps, 64 above),
    the only selected frame in the last lane of the last wave; n = 0 touches nothing."""
    c = TM.cfg(1, flags=TM.F_UDP_CSUM, **FUZZ_CFG[1])
    tun = _load(dp, c)
    rx = _load(dp, TM.cfg(1, **{**FUZZ_CFG[1], "local_ip": 0}))
    for n in (1, 63, 64, 65, 127, 128, 129, 255, 256, 257):
        z = synth.tunnel_fuzz(n, 1, seed=n, stride=S, opt_stride=8, negatives=0)
        sel = np.zeros(n, np.uint8)
        sel[-1] = 1
        kw = dict(opt=z.opt, opt_len=z.opt_len, select=sel, flow_hash=z.flow_hash)
        out, ol, st = _encap(dp, tun, z.frames, z.lens, z.remote_ip, z.tunnel_id, 320, **kw)
        torch.cuda.synchronize()
        w_out, w_ol, w_st = TM.encap_batch(c, z.frames, z.lens, z.remote_ip, z.tunnel_id, 320, **kw)
        assert w_st[-1] == TM.ST_OK and (w_st[:-1] == TM.ST_SKIPPED).all()
        _same_col(_np(st), w_st, f"n={n} status")
        _same_col(_np(ol, np.uint32).reshape(-1), w_ol, f"n={n} out_len")
        _same_rows(_np(out), w_out, f"n={n} rows")
        _same_rx(_decap(dp, rx, out, ol, S, 8), TM.decap_batch(TM.cfg(1, **{**FUZZ_CFG[1], "local_ip": 0}), w_out, w_ol, S, 8),
                 f"n={n} decap")
    from cilium_amd._lib import lib, gf_frames, gf_tunnel_tx, gf_tunnel_rx_out
    tx = gf_tunnel_tx(gf_frames(0, S, None, None), None, None, None, 0, None, None, None, None, None)
    assert lib.gf_tunnel_encap(tun, C.byref(tx), None, 128, None, None, None) == 0
    fr, ro = gf_frames(0, 256, None, None), gf_tunnel_rx_out(None, 64, None, None, None, None, 0, None, None)
    assert lib.gf_tunnel_decap(rx, C.byref(fr), C.byref(ro), None) == 0


# ---------------------------------------------------------------- untouched rows, refusals
def test_gpu_rejected_frames_keep_poison(dp):
    """A batch in which no frame is encapsulated, and one in which none is a tunnel packet: rows and
    columns keep the poison, except status, out_len / inner_len."""
    n, S = 300, 128
    z = synth.tunnel_fuzz(n, 1, seed=9, stride=S, opt_stride=8, negatives=0)
    tun = _load(dp, TM.cfg(1, flags=TM.F_UDP_CSUM, **FUZZ_CFG[1]))
    lens, ol, sel = z.lens.copy(), z.opt_len.copy(), np.ones(n, np.uint8)
    lens[0::4], ol[1::4], sel[2::4] = 13, 6, 0
    lens[3::4] = S + 1
    out, olen, st = _encap(dp, tun, z.frames, lens, z.remote_ip, z.tunnel_id, 256, opt=z.opt, opt_len=ol, select=sel)
    torch.cuda.synchronize()
    assert (_np(st) == np.tile([TM.ST_SHORT, TM.ST_BAD_OPT, TM.ST_SKIPPED, TM.ST_TRUNCATED], n // 4)).all()
    assert (_np(out) == POISON).all() and not _np(olen, np.uint32).any()
    junk = np.random.default_rng(3).integers(0, 256, (n, 256), dtype=np.uint8)
    got = _decap(dp, tun, _dev(junk), _dev(np.full(n, 200), np.uint32), 128, 8)
    assert np.isin(got.status, (TM.ST_NOT_TUNNEL, TM.ST_BAD_OUTER)).all() and not got.inner_len.any()
    assert (got.inner == POISON).all() and (got.opt == POISON).all() and (got.opt_len == POISON).all()
    assert (got.tunnel_id == P32).all() and (got.outer_saddr == P32).all()


def test_gpu_refusals_leave_the_outputs_alone(dp):
    from cilium_amd._lib import lib, gf_frames, gf_tunnel_tx
    n = 8
    z = synth.tunnel_fuzz(n, 0, seed=1, stride=128, negatives=0)
    tun = _load(dp, TM.cfg(0, **FUZZ_CFG[0]))
    f, ln, rip, tid = _dev(z.frames), _dev(z.lens, np.uint32), _dev(z.remote_ip, np.uint32), _dev(z.tunnel_id, np.uint32)
    out = torch.full((n, 128), POISON, dtype=torch.uint8, device="cuda")
    ol = torch.full((n, 4), POISON, dtype=torch.uint8, device="cuda")
    st = torch.full((n,), POISON, dtype=torch.uint8, device="cuda")
    mk = lambda stride=128, rip_=rip.data_ptr(): gf_tunnel_tx(gf_frames(n, stride, f.data_ptr(), ln.data_ptr()), rip_,
                                                              tid.data_ptr(), None, 0, None, None, None, None, None)
    call = lambda h, b, o=out.data_ptr(), os_=128: lib.gf_tunnel_encap(h, C.byref(b), o, os_, ol.data_ptr(), st.data_ptr(), None)
    assert call(dp.tunnel_load(1, 6081) + 1000, mk()) == -errno.EBADF
    assert call(tun, mk(rip_=None)) == -errno.EFAULT
    assert call(tun, mk(stride=257)) == -errno.EINVAL and call(tun, mk(), os_=96) == -errno.EINVAL
    assert call(tun, mk(), o=out.data_ptr() + 4) == -errno.EINVAL and call(tun, mk(), o=f.data_ptr()) == -errno.EINVAL
    torch.cuda.synchronize()
    assert (_np(out) == POISON).all() and (_np(ol) == POISON).all() and (_np(st) == POISON).all()


# ---------------------------------------------------------------- gf_tunnel_select
def test_gpu_select(dp):
    from cilium_amd.datapath import EG_OUT, PIPE_OUT
    from cilium_amd._lib import GF_REC_EGRESS, GF_REC_PIPELINE
    rng = np.random.default_rng(4)
    n = 1000
    eg = np.zeros(n, EG_OUT)
    eg["eg_flags"] = rng.integers(0, 1 << 16, n)
    eg["action"] = rng.integers(0, 8, n)
    sel = dp.tunnel_select(GF_REC_EGRESS, _dev(eg.view(np.uint8).reshape(n, 24)))
    pi = np.zeros(n, PIPE_OUT)
    pi["action"] = rng.choice([0, 2, 7], n)
    pi["ifindex_lo"] = rng.choice([0, 3, 7, 7 + 256], n)
    pi["flags"] = rng.integers(0, 256, n)
    sel2 = dp.tunnel_select(GF_REC_PIPELINE, _dev(pi.view(np.uint8).reshape(n, 24)))
    torch.cuda.synchronize()
    assert np.array_equal(_np(sel), ((eg["eg_flags"] & 0x40) != 0).astype(np.uint8))
    want2 = ((pi["action"] == 7) & (pi["ifindex_lo"] == 7)).astype(np.uint8)      # ENCAP_IFINDEX of the fixture's node
    assert np.array_equal(_np(sel2), want2) and 50 < want2.sum() < n - 50


# ---------------------------------------------------------------- the chain across two nodes
class Ring:
    def __init__(self, cap):
        from cilium_amd._lib import lib, gf_event_ring
        self.lib, self.cap = lib, cap
        self.recs = torch.zeros((cap, 160), dtype=torch.uint8, device="cuda")
        self.cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
        self.ring = gf_event_ring(self.recs.data_ptr(), cap, self.cnt.data_ptr())

    def __enter__(self):
        assert self.lib.gf_set_event_ring(C.byref(self.ring)) == 0
        return self

    def __exit__(self, *a):
        self.lib.gf_set_event_ring(None)

    def raw(self):
        torch.cuda.synchronize()
        n = int(self.cnt.item())
        return n, self.recs[:min(n, self.cap)].cpu().numpy()


@pytest.mark.parametrize("mode", [0, 1], ids=["vxlan", "geneve"])
def test_gpu_chain_two_nodes(mode):
    """gf_lxc_egress_classify -> gf_lxc_egress_tunnel_meta -> gf_tunnel_select -> gf_tunnel_encap on
    node A, the selected outer frames -> gf_tunnel_decap -> gf_overlay_classify_opts on node B:
    records, snap_out and the event ring equal those of node B fed the inner frames and the
    metadata directly."""
    _gpu()
    from cilium_amd.datapath import Datapath, DeviceBatch
    from cilium_amd._lib import GF_REC_EGRESS
    from tests.test_geneve import two_node_scenarios, F_GENEVE, F_TRACE
    scA, scB, ro, rs = two_node_scenarios()
    scB.overlay = {"lxc_map": "cilium_lxc", "flags": (F_GENEVE if mode else 0) | F_TRACE, "ingress_ifindex": 9}
    pkA = scA.batches[0]
    S = pkA.frames.shape[1]
    csum = bool((pkA.lens <= S).all())
    nodeA, nodeB = synth.ip4("192.168.10.1"), 0     # node B accepts any destination: A's tunnel map names many nodes
    dps = []
    try:
        dpA = Datapath(scA, pin_prefix=None)
        dps.append(dpA)
        bA = DeviceBatch(pkA, parse=False)
        out, snap = dpA.egress(bA, scA.now)
        tid, opt, ol = dpA.egress_tunnel_meta(bA.lxc_id, out)
        sel = dpA.tunnel_select(GF_REC_EGRESS, out)
        rip = out[:, 16:20].contiguous().view(torch.int32).reshape(-1)          # gf_egress_out.tunnel_ip
        tunA = dpA.tunnel_load(mode, 6081 if mode else 8472, nodeA, TM.F_UDP_CSUM if csum else 0,
                               src_mac=bytes.fromhex("0200000a0001"), dst_mac=bytes.fromhex("020000140002"))
        OS = 512 if S > 128 else 256
        outer, olen, st = dpA.tunnel_encap(tunA, snap, bA.len, rip, tid, OS, opt=opt, opt_len=ol, select=sel,
                                           flow_hash=bA.flow_hash)
        idx = sel.nonzero().squeeze(1)
        torch.cuda.synchronize()
        enc = ro["eg_flags"] & 0x40 != 0
        assert np.array_equal(_np(sel), enc.astype(np.uint8)) and enc.sum() >= 200
        assert (_np(st)[enc] == TM.ST_OK).all() and (_np(st)[~enc] == TM.ST_SKIPPED).all()
        wire, wlen = outer[idx].contiguous(), olen[idx].contiguous()
        # the inner frames and metadata, directly: the bytes inside len, as the tunnel carries them
        lens = bA.len[idx].contiguous()
        inside = torch.arange(S, device="cuda")[None, :] < lens[:, None]
        direct = types.SimpleNamespace(n=int(idx.numel()), device="cuda", frames=(snap[idx] * inside).contiguous(), len=lens,
                                       tunnel_id=(tid[idx] & 0xffffff).contiguous(), tc_index=None, flow_hash=None)
        d_opt, d_ol = opt[idx].contiguous(), ol[idx].contiguous()
        res = []
        for via_wire in (True, False):
            dpB = Datapath(scB, pin_prefix=None)
            dps.append(dpB)
            with Ring(1 << 15) as ring:
                if via_wire:
                    tunB = dpB.tunnel_load(mode, 6081 if mode else 8472, nodeB)
                    b = dpB.tunnel_decap(tunB, wire, wlen, inner_stride=S, opt_stride=8)
                    torch.cuda.synchronize()
                    assert (_np(b.status) == TM.ST_OK).all()
                    assert torch.equal(b.frames, direct.frames) and torch.equal(b.len, direct.len)
                    assert torch.equal(b.tunnel_id, direct.tunnel_id) and (_np(b.outer_saddr, np.uint32) == nodeA).all()
                    if mode:
                        assert torch.equal(b.opt, d_opt) and torch.equal(b.opt_len, d_ol)
                    o, s = dpB.overlay(b, scB.now, opt=b.opt, opt_len=b.opt_len) if mode else dpB.overlay(b, scB.now)
                else:
                    o, s = dpB.overlay(direct, scB.now, opt=d_opt, opt_len=d_ol) if mode else dpB.overlay(direct, scB.now)
                res.append((_np(o).copy(), _np(s).copy(), ring.raw()))
            dpB.close()
        (o1, s1, (n1, r1)), (o2, s2, (n2, r2)) = res
        assert np.array_equal(o1, o2) and np.array_equal(s1, s2)
        assert n1 == n2 >= direct.n and np.array_equal(r1, r2)
        assert (o1[:, 0] == 4).sum() >= 100                                      # tail-called into handle_policy
    finally:
        for d in dps:
            d.close()
