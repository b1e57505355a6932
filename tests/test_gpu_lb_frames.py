"""gf_lb_classify_frames (k_lb_frames) on the GPU: bpf_lb's from-netdev over raw frames against
the hand-derived KATs, gf_lb_classify on the parsed columns, tests/lb_frames_model.py (anchored
on the oracle in tests/test_lb_frames.py), the oracle's pipeline at GF_STAGE_LB and the drop
records of gf_pipeline_classify."""
import ctypes as C
import errno

import numpy as np
import pytest

from cilium_amd import synth
from oracle.scenario import OracleDP
from tests import lb_frames_model as LM

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DOC = LM.load_kats()
MAC = bytes.fromhex("aabbccddeeff")
STAGE_XDP, STAGE_LB = 1, 2


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(0)


class Ring:
    def __init__(self, cap):
        from cilium_amd._lib import lib, gf_event_ring
        self.lib, self.cap = lib, cap
        self.recs = torch.zeros((max(cap, 1), 160), dtype=torch.uint8, device="cuda")
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


def _run(dp, pk, mode):
    """mode: "out" (a fresh buffer), "inplace", "null".  Returns (records LB_OUT, nd6, frames as
    left or None, the input frames after the call)."""
    from cilium_amd.datapath import DeviceBatch, LB_OUT, to_numpy
    b = DeviceBatch(pk, parse=False)
    out, nd6, snap = dp.lb_frames(b, snap_out={"out": True, "inplace": "inplace", "null": False}[mode])
    torch.cuda.synchronize()
    return (to_numpy(out, LB_OUT), nd6.cpu().numpy(), None if snap is None else snap.cpu().numpy(),
            b.frames.cpu().numpy())


def _same_recs(got, want, what):
    bad = np.nonzero(got.view(np.uint8).reshape(-1, 12) != want.view(np.uint8).reshape(-1, 12))[0]
    assert not len(bad), (what, int(bad[0]), got[bad[0]], want[bad[0]])


def _same_frames(got, want, what):
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert not len(bad), (what, int(bad[0]), np.nonzero(got[bad[0]] != want[bad[0]])[0])


def _cut(pk, n, stride):
    """The first n frames of pk under a snap of `stride` bytes (the wire lengths stay)."""
    p = pk.slice(0, n)
    return synth.Packets(np.ascontiguousarray(p.frames[:, :stride]), p.lens, flow_hash=p.flow_hash)


@pytest.fixture(scope="module")
def fuzz():
    """(scenario with LB_REDIRECT, its first batch)"""
    sc = synth.lb_frames_fuzz(seed=3, n_packets=4096, n_batches=1)
    return sc, sc.batches[0]


def _variant(sc, redirect, dstmac):
    import copy
    v = copy.copy(sc)
    fl = sc.lb["flags"] | synth.LB_REDIRECT if redirect else sc.lb["flags"] & ~synth.LB_REDIRECT
    v.lb = {k: x for k, x in sc.lb.items() if k != "dstmac"}
    v.lb["flags"] = fl
    if dstmac:
        v.lb["dstmac"] = MAC
    return v


@pytest.mark.parametrize("mode", ["out", "inplace"])
def test_kats(mode):
    _gpu()
    from cilium_amd.datapath import Datapath
    for (flags, dstmac), kats in LM.kat_groups(DOC):
        dp = Datapath(LM.kat_scenario(DOC, flags, dstmac), pin_prefix=None)
        try:
            pk, recs, nd6, out = LM.kat_packets(DOC, kats)
            r, n6, snap, _ = _run(dp, pk, mode)
            names = [k["name"] for k in kats]
            _same_recs(r, recs, names)
            assert np.array_equal(n6, nd6), names
            _same_frames(snap, out, names)
        finally:
            dp.close()


def test_records_equal_lb_classify_on_parsed_columns(fuzz):
    _gpu()
    from cilium_amd.datapath import Datapath, DeviceBatch, LB_OUT, to_numpy
    sc, pk = fuzz
    et = (pk.frames[:, 12].astype(int) << 8) | pk.frames[:, 13]
    assert (et == 0x0800).sum() > 1000 and (et == 0x86DD).sum() > 200
    for redirect in (True, False):
        dp = Datapath(_variant(sc, redirect, False), pin_prefix=None)
        try:
            b = DeviceBatch(pk)
            lo, ln6 = dp.lb(b)
            fo, fn6, _ = dp.lb_frames(b, snap_out=False)
            torch.cuda.synchronize()
            assert torch.equal(lo, fo) and torch.equal(ln6, fn6)
            r = to_numpy(fo, LB_OUT)
            assert (r["slave"] != 0).sum() * 4 >= pk.n and (r["action"] == LM.TC_ACT_SHOT).any()
            assert ((r["action"] == LM.TC_ACT_REDIRECT).any()) == redirect
        finally:
            dp.close()


@pytest.mark.parametrize("redirect", [True, False], ids=["redirect", "noredirect"])
@pytest.mark.parametrize("dstmac", [True, False], ids=["dstmac", "nomac"])
def test_frames_and_records_equal_model(fuzz, redirect, dstmac):
    """{REDIRECT, no REDIRECT} x {DSTMAC, none} x {in place, out of place, snap_out NULL}.  LB_DSTMAC
    without LB_REDIRECT cannot be configured (-EINVAL): that program runs without it."""
    _gpu()
    from cilium_amd._lib import lib
    from cilium_amd.datapath import Datapath
    sc, pk = fuzz
    v = _variant(sc, redirect, dstmac and redirect)
    dp = Datapath(v, pin_prefix=None)
    try:
        if dstmac and not redirect:
            assert lib.gf_lb_prog_set_dstmac(dp.lb_prog, (C.c_uint8 * 6)(*MAC)) == -errno.EINVAL
        mr, mn6, mf = LM.LbFramesModel(v).batch(pk)
        assert (mr["slave"] != 0).sum() * 4 >= pk.n
        if dstmac and redirect:
            assert (mf[:, :6] != pk.frames[:, :6]).any()
        r, n6, snap, inp = _run(dp, pk, "out")
        _same_recs(r, mr, "out")
        assert np.array_equal(n6, mn6)
        _same_frames(snap, mf, "out")
        assert np.array_equal(inp, pk.frames)           # out of place leaves the input alone
        same = mr["slave"] == 0
        assert np.array_equal(snap[same], pk.frames[same])   # untouched frames copied verbatim
        r2, n62, snap2, inp2 = _run(dp, pk, "inplace")
        _same_recs(r2, r, "inplace")
        assert np.array_equal(n62, n6)
        _same_frames(snap2, snap, "inplace == out of place")
        assert np.array_equal(inp2, snap2)
        r3, n63, snap3, inp3 = _run(dp, pk, "null")
        _same_recs(r3, r, "null")
        assert np.array_equal(n63, n6) and snap3 is None and np.array_equal(inp3, pk.frames)
    finally:
        dp.close()


def test_equal_to_oracle_pipeline_at_stage_lb(fuzz):
    _gpu()
    from cilium_amd.datapath import Datapath
    sc, pk = fuzz
    ro, rn6, rs = OracleDP(sc).pipeline(pk, sc.now)
    dp = Datapath(sc, pin_prefix=None)
    try:
        r, n6, snap, _ = _run(dp, pk, "out")
    finally:
        dp.close()
    lb = ro["stage"] == STAGE_LB
    assert np.array_equal(lb, (r["action"] == LM.TC_ACT_SHOT) | (r["action"] == LM.TC_ACT_REDIRECT))
    assert np.array_equal(r["action"][lb], ro["action"][lb]) and np.array_equal(r["reason"][lb], ro["reason"][lb])
    rd = lb & (ro["action"] == LM.TC_ACT_REDIRECT)
    for a, b in (("slave", "slave"), ("rev_nat", "rev_nat"), ("new_dport", "dport"), ("new_daddr4", "daddr4")):
        assert np.array_equal(r[a][rd], ro[b][rd]), a
    assert np.array_equal(n6[rd], rn6[rd])
    _same_frames(snap[rd], rs[rd], "redirected frames")
    assert rd.sum() * 4 >= pk.n and set(ro["reason"][lb & ~rd]) == {14, 134, 154, 158}


def test_drop_records_equal_pipeline(fuzz):
    """send_drop_notify_error's records: byte for byte gf_pipeline_classify's for the frames it
    drops at GF_STAGE_LB; a ring smaller than the number of drops keeps the first ones and counts all."""
    _gpu()
    from cilium_amd.datapath import Datapath, DeviceBatch, PIPE_OUT, to_numpy
    sc, pk = fuzz
    dp = Datapath(sc, pin_prefix=None)
    try:
        with Ring(8192) as ring:
            out, _, _ = dp.pipeline(DeviceBatch(pk, parse=False), sc.now)
            n_pipe, ev_pipe = ring.raw()
        po = to_numpy(out, PIPE_OUT)
        shot = np.nonzero((po["action"] == LM.TC_ACT_SHOT) & (po["stage"] != STAGE_XDP))[0]
        assert n_pipe == len(shot) == len(ev_pipe)      # nothing in this scenario traces
        want = ev_pipe[po["stage"][shot] == STAGE_LB]
        for mode in ("out", "inplace", "null"):
            with Ring(8192) as ring:
                r, _, _, _ = _run(dp, pk, mode)
                n_lb, ev_lb = ring.raw()
            drops = int((r["action"] == LM.TC_ACT_SHOT).sum())
            assert n_lb == drops == len(want) > 20, mode
            assert np.array_equal(ev_lb, want), mode
        assert np.array_equal(want, LM.drop_events(pk, r, pk.frames))
        small = len(want) // 3
        with Ring(small) as ring:
            _run(dp, pk, "out")
            n_lb, ev_lb = ring.raw()
        assert n_lb == len(want) and np.array_equal(ev_lb, want[:small])
    finally:
        dp.close()


def test_stats_sink_counts_the_call(fuzz):
    _gpu()
    from cilium_amd._lib import lib
    from cilium_amd.datapath import Datapath
    sc, pk = fuzz
    dp = Datapath(sc, pin_prefix=None)
    cnt = torch.zeros(512, dtype=torch.int64, device="cuda")
    lib.gf_set_stats_sink(C.c_void_p(cnt.data_ptr()))
    try:
        r, _, _, _ = _run(dp, pk, "out")
    finally:
        lib.gf_set_stats_sink(None)
        dp.close()
    c = cnt.cpu().numpy()
    assert c[268] == pk.n and c[269] == np.asarray(pk.lens, np.int64).sum()
    for a in np.unique(r["action"]):
        assert c[256 + int(a)] == (r["action"] == a).sum(), a
    for x in range(1, 256):
        assert c[x] == (r["reason"] == x).sum(), x


def test_error_codes_leave_maps_and_frames_alone(fuzz):
    _gpu()
    from cilium_amd._lib import lib, gf_frames
    from cilium_amd.datapath import Datapath, DeviceBatch
    sc, pk = fuzz
    dp = Datapath(sc, pin_prefix=None)
    try:
        b = DeviceBatch(pk.slice(0, 300), parse=False)
        before = {n: dp.dump_map(n) for n in ("lb4_svc", "lb6_svc")}
        frames0 = b.frames.clone()
        S = b.frames.shape[1]
        out = torch.full((b.n, 12), 0xa5, dtype=torch.uint8, device="cuda")
        nd6 = torch.full((b.n, 16), 0xa5, dtype=torch.uint8, device="cuda")
        snap = torch.full_like(b.frames, 0xa5)
        p = lambda t: None if t is None else t.data_ptr()

        def call(prog, n=b.n, stride=S, fr_snap=b.frames, fr_len=b.len, o=out, so=snap, frames=True):
            fr = gf_frames(n, stride, p(fr_snap), p(fr_len))
            return lib.gf_lb_classify_frames(prog, C.byref(fr) if frames else None, p(b.flow_hash), p(o), p(nd6), p(so), None)

        with Ring(64) as ring:
            assert call(0) == -errno.EBADF
            assert call(987654) == -errno.EBADF
            assert call(dp.fd["lb4_svc"]) == -errno.EBADF           # a map is not an LB program
            assert call(dp.pipe) == -errno.EBADF
            assert call(dp.lb_prog, frames=False) == -errno.EFAULT
            assert call(dp.lb_prog, o=None) == -errno.EFAULT
            assert call(dp.lb_prog, fr_snap=None) == -errno.EFAULT
            assert call(dp.lb_prog, fr_len=None) == -errno.EFAULT
            assert call(dp.lb_prog, n=0, o=None, fr_snap=None, fr_len=None) == 0
            assert call(dp.lb_prog, stride=13) == -errno.EINVAL
            assert call(dp.lb_prog, stride=257) == -errno.EINVAL
            assert call(dp.lb_prog, n=(1 << 30) + 1) == -errno.E2BIG
            n_ev, _ = ring.raw()
        torch.cuda.synchronize()
        assert n_ev == 0
        assert torch.equal(b.frames, frames0)
        for t in (out, nd6, snap):
            assert bool((t == 0xa5).all())
        assert {n: dp.dump_map(n) for n in before} == before
        assert call(dp.lb_prog) == 0                    # and the same arguments run
        torch.cuda.synchronize()
        assert not bool((out == 0xa5).all())
    finally:
        dp.close()


def test_set_dstmac_errors_and_undefine(fuzz):
    _gpu()
    from cilium_amd._lib import lib
    from cilium_amd.datapath import Datapath
    sc, pk = fuzz
    mac = (C.c_uint8 * 6)(*MAC)
    dp = Datapath(_variant(sc, True, False), pin_prefix=None)
    dp2 = Datapath(_variant(sc, False, False), pin_prefix=None)
    try:
        assert lib.gf_lb_prog_set_dstmac(0, mac) == -errno.EBADF
        assert lib.gf_lb_prog_set_dstmac(dp.fd["lb4_svc"], mac) == -errno.EBADF
        assert lib.gf_lb_prog_set_dstmac(dp.policy_array, mac) == -errno.EBADF
        assert lib.gf_lb_prog_set_dstmac(dp2.lb_prog, mac) == -errno.EINVAL
        assert lib.gf_lb_prog_set_dstmac(dp2.lb_prog, None) == -errno.EINVAL
        p = pk.slice(0, 700)
        r0, _, f0, _ = _run(dp, p, "out")
        assert lib.gf_lb_prog_set_dstmac(dp.lb_prog, mac) == 0
        r1, _, f1, _ = _run(dp, p, "out")
        rd = r1["action"] == LM.TC_ACT_REDIRECT
        _same_recs(r1, r0, "records do not depend on LB_DSTMAC")
        assert rd.any() and (f1[rd, :6] == np.frombuffer(MAC, np.uint8)).all()
        assert np.array_equal(f1[:, 6:], f0[:, 6:]) and np.array_equal(f1[~rd], f0[~rd])
        assert lib.gf_lb_prog_set_dstmac(dp.lb_prog, None) == 0
        r2, _, f2, _ = _run(dp, p, "out")
        assert np.array_equal(f2, f0)
    finally:
        dp.close()
        dp2.close()


@pytest.mark.parametrize("stride", [64, 128, 256])
def test_shapes(fuzz, stride):
    """n in {0, 1, 63, 64, 65, 257, 4096}: a partial wave, a full one, one lane more, a second
    block with one frame (256 lanes a block at strides up to 128, 128 at 256), many blocks."""
    _gpu()
    from cilium_amd.datapath import Datapath
    sc, pk = fuzz
    v = _variant(sc, True, True)
    full = _cut(pk, 4096, stride)
    mr, mn6, mf = LM.LbFramesModel(v).batch(full)
    assert (mr["slave"] != 0).sum() > 500
    dp = Datapath(v, pin_prefix=None)
    try:
        for n in (0, 1, 63, 64, 65, 257, 4096):
            p = _cut(pk, n, stride)
            for mode in ("out", "inplace"):
                r, n6, snap, _ = _run(dp, p, mode)
                assert len(r) == n
                _same_recs(r, mr[:n], (n, mode))
                assert np.array_equal(n6, mn6[:n]), (n, mode)
                _same_frames(snap, mf[:n], (n, mode))
    finally:
        dp.close()


@pytest.mark.parametrize("mode", ["out", "inplace"])
def test_only_last_frame_of_last_wave_translated(mode):
    _gpu()
    from cilium_amd.datapath import Datapath
    by_name = {k["name"]: k for k in DOC["kats"]}
    n = 256 + 64                                        # the last lane of the second block's only wave
    kats = [by_name["arp"]] * (n - 1) + [by_name["v4_tcp_l4_redirect_dstmac"]]
    pk, recs, nd6, out = LM.kat_packets(DOC, kats)
    k = by_name["v4_tcp_l4_redirect_dstmac"]
    dp = Datapath(LM.kat_scenario(DOC, k["flags"], k["dstmac"]), pin_prefix=None)
    try:
        r, n6, snap, _ = _run(dp, pk, mode)
        _same_recs(r, recs, mode)
        _same_frames(snap, out, mode)
        assert r["action"][-1] == LM.TC_ACT_REDIRECT and not r["action"][:-1].any()
        assert np.array_equal(snap[:-1], pk.frames[:-1]) and not np.array_equal(snap[-1], pk.frames[-1])
    finally:
        dp.close()
