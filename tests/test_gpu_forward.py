"""gf_forward_queues / gf_forward_frames on the GPU (k_fwd_queues, k_fwd_count, k_fwd_scan,
k_fwd_scatter) against tests/forward_model.py, bit for bit: the queue column from the device
records of the classify calls, and qoff, counts and the packed rows, lengths and indices of the
partition.  Every output buffer is pre-filled with 0xA5 and carries guard rows past max_out;
whatever lies at or past row counts[2] must still be 0xA5 after the call.

The three launches of gf_forward_frames run one block per tile (no grid cap, no grid-stride loop),
so there is no several-tiles-per-block case to force here."""
import ctypes as C
import errno

import numpy as np
import pytest

from tests import forward_model as M

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

GUARD = 8            # rows past max_out in every output buffer
DROP = M.DROP


@pytest.fixture(scope="module", autouse=True)
def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(0)


def _batch(n, stride, seed=1):
    """n rows of random bytes (the call never looks inside a row) and wire lengths on both sides of the snap."""
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (n, stride), dtype=np.uint8), rng.integers(14, 1515, n).astype(np.uint32)


def _dev_rows(frames, odd=False):
    f = torch.from_numpy(np.ascontiguousarray(frames))
    if not odd:
        return f.cuda()
    buf = torch.empty(f.numel() + 1, dtype=torch.uint8, device="cuda")
    t = buf[1:].view(f.shape)
    t.copy_(f)
    assert t.data_ptr() % 2 == 1
    return t


def _i32(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.uint32)).view(np.int32)).cuda()


class Fwd:
    """One gf_forward_frames call through the C ABI over device tensors, every output pre-filled with 0xA5."""

    def __init__(self, frames, lens, queue, nq, max_out=None, snap=True, index=True, odd=False, odd_out=False):
        from cilium_amd._lib import lib, gf_frames, gf_forward_out
        n, stride = frames.shape
        self.frames, self.lens, self.queue, self.nq, self.n = frames, lens, np.asarray(queue, np.uint8), nq, n
        self.max_out = n if max_out is None else max_out
        self.d_frames, self.d_len, self.d_queue = _dev_rows(frames, odd), _i32(lens), torch.from_numpy(self.queue.copy()).cuda()
        full = lambda *shape: torch.full(shape, 0xa5, dtype=torch.uint8, device="cuda")
        rows = self.max_out + GUARD
        self.snap = None
        if snap:
            self.snap = full(rows * stride + 1)[1:].view(rows, stride) if odd_out else full(rows, stride)
        self.len = full(rows, 4) if snap else None
        self.index = full(rows, 4) if snap and index else None
        self.qoff, self.counts = full(nq + 1 + GUARD, 4), full(4 + GUARD, 4)
        p = lambda t: None if t is None else t.data_ptr()
        fr = gf_frames(n, stride, self.d_frames.data_ptr(), self.d_len.data_ptr())
        o = gf_forward_out(p(self.snap), p(self.len), p(self.index), self.max_out, p(self.qoff), p(self.counts))
        self.rc = lib.gf_forward_frames(C.byref(fr), self.d_queue.data_ptr(), nq, C.byref(o),
                                        C.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()

    @staticmethod
    def np32(t):
        return t.cpu().numpy().view(np.uint32).ravel()

    def check(self, what):
        assert self.rc == 0, what
        m = M.partition(self.frames, self.lens, self.queue, self.nq, self.max_out, snap=self.snap is not None)
        w = m["written"]
        assert self.np32(self.qoff)[:self.nq + 1].tolist() == m["qoff"].tolist(), (what, "qoff")
        assert self.np32(self.counts)[:4].tolist() == m["counts"], (what, "counts")
        assert (self.qoff.cpu().numpy()[self.nq + 1:] == 0xa5).all() and (self.counts.cpu().numpy()[4:] == 0xa5).all(), what
        assert np.array_equal(self.d_frames.cpu().numpy(), self.frames), (what, "the input was written")
        assert np.array_equal(self.d_queue.cpu().numpy(), self.queue), (what, "the queue column was written")
        if self.snap is None:
            return m
        snap = self.snap.cpu().numpy()
        bad = np.nonzero((snap[:w] != m["snap"]).any(axis=1))[0]
        assert not len(bad), (what, "row", int(bad[0]))
        assert np.array_equal(self.np32(self.len)[:w], m["len"]), (what, "len")
        assert (snap[w:] == 0xa5).all() and (self.len.cpu().numpy()[w:] == 0xa5).all(), (what, "written past counts[2]")
        if self.index is not None:
            assert np.array_equal(self.np32(self.index)[:w], m["index"]), (what, "index")
            assert (self.index.cpu().numpy()[w:] == 0xa5).all(), (what, "index written past counts[2]")
        return m


def _random_queue(n, nq, seed, drop=0.2):
    rng = np.random.default_rng(seed)
    q = rng.integers(0, nq, n).astype(np.uint8)
    q[rng.random(n) < drop] = DROP
    return q


# ------------------------------------------------------------------ sizes and queue counts
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1023, 1024, 1025, 2049])
def test_batch_sizes(n):
    """A partial wave, a full one, one lane more; a tile less one frame, a full tile, a second tile
    with one frame, a third with one.  Five queues and GF_FWD_DROP at random."""
    f, ln = _batch(n, 64, n)
    Fwd(f, ln, _random_queue(n, 5, n), 5).check(n)


@pytest.mark.parametrize("nq", [1, 2, 3, 64])
def test_queue_counts(nq):
    """2,500 rows (three tiles) over nq queues.  nq = 64: the first wave holds every queue once and
    the second every queue once in reverse, so each lane's set of peers is itself."""
    n = 2500
    f, ln = _batch(n, 64, nq)
    q = _random_queue(n, nq, 100 + nq)
    if nq == 64:
        q[:64] = np.random.default_rng(9).permutation(64)
        q[64:128] = np.arange(63, -1, -1)
    m = Fwd(f, ln, q, nq).check(nq)
    if nq == 64:
        assert (np.diff(m["qoff"].astype(np.int64)) > 0).all()            # every queue is in use


def test_queue_patterns():
    """One tile and a half.  A queue whose rows span all waves of a tile, one row a wave, among rows
    of the other queues; a queue that stays empty; every row dropped; every row in one queue."""
    n = 1536
    f, ln = _batch(n, 64, 3)
    q = np.random.default_rng(5).integers(1, 4, n).astype(np.uint8)       # queues 1..3
    q[5::64] = 0                                                          # queue 0: lane 5 of every wave
    m = Fwd(f, ln, q, 5).check("spanning")                                # queue 4 is empty
    assert m["qoff"][1] == n // 64 and m["qoff"][4] == m["qoff"][5] == n
    q2 = q.copy()
    q2[q2 == 2] = DROP
    m = Fwd(f, ln, q2, 5).check("an empty queue in the middle")
    assert m["qoff"][2] == m["qoff"][3] and m["counts"][1] > 0
    m = Fwd(f, ln, np.full(n, DROP, np.uint8), 4).check("all dropped")
    assert m["counts"] == [0, n, 0, 0]
    for one in (0, 3):
        m = Fwd(f, ln, np.full(n, one, np.uint8), 4).check(("all in queue", one))
        assert m["counts"] == [n, 0, n, 0] and np.array_equal(m["order"], np.arange(n))


@pytest.mark.parametrize("stride", [14, 34, 64, 68, 67, 128, 256])
def test_strides(stride):
    """64 / 128 / 256: 16-byte pieces; 68: 4-byte pieces (rows not 16-byte aligned); 14, 34 and 67: byte
    pieces.  At an odd base address of the input or of the output every stride moves byte by byte."""
    n = 1300
    f, ln = _batch(n, stride, stride)
    q = _random_queue(n, 5, stride)
    Fwd(f, ln, q, 5).check(stride)
    if stride in (14, 64, 68):
        Fwd(f, ln, q, 5, odd=True).check((stride, "odd input address"))
    if stride == 64:
        Fwd(f, ln, q, 5, odd_out=True).check((stride, "odd output address"))


# ------------------------------------------------------------------ capacity, invalid bytes, optional outputs
def test_capacity():
    """max_out in {0, 1, a cut inside queue 1, the forwarded count} over 2,500 rows: qoff and
    counts[0] stay, the first max_out rows of the queue-major order are written, 0xA5 elsewhere."""
    n = 2500
    f, ln = _batch(n, 64, 7)
    q = _random_queue(n, 4, 7)
    full = M.partition(f, ln, q, 4)
    k = full["counts"][0]
    cut = int(full["qoff"][1] + full["qoff"][2]) // 2
    assert full["qoff"][1] < cut < full["qoff"][2] and 1024 < k < n
    for mo in (0, 1, cut, k - 1, k):
        m = Fwd(f, ln, q, 4, max_out=mo).check(("max_out", mo))
        assert m["qoff"].tolist() == full["qoff"].tolist() and m["counts"][0] == k and m["counts"][2] == min(k, mo)


def test_invalid_queue_bytes():
    """Bytes >= n_queues other than GF_FWD_DROP are not forwarded and are counted in counts[3]."""
    n = 1500
    f, ln = _batch(n, 64, 8)
    q = _random_queue(n, 3, 8)
    q[7::13] = 3                                                          # n_queues itself
    q[3::29] = 64
    q[11::31] = 0xfe
    m = Fwd(f, ln, q, 3).check("invalid")
    inv = int(((q >= 3) & (q != DROP)).sum())
    assert m["counts"][3] == inv > 150 and m["counts"][1] == inv + int((q == DROP).sum())
    m = Fwd(f, ln, np.full(n, 64, np.uint8), 64).check("64 with 64 queues")
    assert m["counts"] == [0, n, 0, n]


def test_optional_outputs():
    n = 2500
    f, ln = _batch(n, 128, 9)
    q = _random_queue(n, 6, 9)
    m = Fwd(f, ln, q, 6, snap=False).check("snap NULL")                   # counts only
    assert m["counts"][2] == 0 and m["counts"][0] > 0
    Fwd(f, ln, q, 6, index=False).check("index NULL")
    Fwd(f, ln, q, 6, index=False, max_out=100).check("index NULL, cut")


def test_launches():
    """Three launches with rows to write; without snap, or with max_out 0, the scatter is not launched."""
    from cilium_amd._lib import lib, gf_prof_rec
    f, ln = _batch(1500, 64, 2)
    q = _random_queue(1500, 4, 2)

    def launched(**kw):
        recs = (gf_prof_rec * 32)()
        lib.gf_prof_enable(1)
        try:
            Fwd(f, ln, q, 4, **kw).check(kw)
            k = lib.gf_prof_read(recs, 32)
        finally:
            lib.gf_prof_enable(0)
        return {recs[j].name.decode() for j in range(k)} & {"k_fwd_queues", "k_fwd_count", "k_fwd_scan", "k_fwd_scatter"}

    assert launched() == {"k_fwd_count", "k_fwd_scan", "k_fwd_scatter"}
    assert launched(snap=False) == launched(max_out=0) == {"k_fwd_count", "k_fwd_scan"}


# ------------------------------------------------------------------ refusals
def test_refusals_write_nothing_and_empty_batch():
    from cilium_amd._lib import lib, gf_frames, gf_forward_cfg, gf_forward_out
    n = 300
    f, ln = _batch(n, 64, 4)
    q = _random_queue(n, 4, 4)
    df, dl, dq = _dev_rows(f), _i32(ln), torch.from_numpy(q.copy()).cuda()
    full = lambda *shape: torch.full(shape, 0xa5, dtype=torch.uint8, device="cuda")
    snap, olen, oidx, qoff, counts = full(n, 64), full(n, 4), full(n, 4), full(65, 4), full(4, 4)
    outs = (snap, olen, oidx, qoff, counts)

    def call(n=n, stride=64, fs=df.data_ptr(), fl=dl.data_ptr(), qu=dq.data_ptr(), nq=4, s=snap.data_ptr(),
             l=olen.data_ptr(), i=oidx.data_ptr(), m=n, qo=qoff.data_ptr(), c=counts.data_ptr(), frames=True, out=True):
        fr, o = gf_frames(n, stride, fs, fl), gf_forward_out(s, l, i, m, qo, c)
        return lib.gf_forward_frames(C.byref(fr) if frames else None, qu, nq, C.byref(o) if out else None, None)

    EFAULT, EINVAL = -errno.EFAULT, -errno.EINVAL
    assert call(frames=False) == EFAULT and call(qu=None) == EFAULT and call(out=False) == EFAULT
    assert call(qo=None) == EFAULT and call(c=None) == EFAULT
    assert call(fs=None) == EFAULT and call(fl=None) == EFAULT and call(l=None) == EFAULT
    assert call(nq=0) == EINVAL and call(nq=65) == EINVAL
    assert call(stride=13) == EINVAL and call(stride=257) == EINVAL
    assert call(s=None) == EINVAL and call(s=None, l=None) == EINVAL
    assert call(s=df.data_ptr()) == EINVAL and call(s=df.data_ptr() + 64 * (n - 1)) == EINVAL
    assert call(l=dl.data_ptr()) == EINVAL and call(i=dq.data_ptr()) == EINVAL and call(s=dq.data_ptr() + n - 1) == EINVAL
    assert call(qo=dq.data_ptr()) == EINVAL and call(c=df.data_ptr() + 7) == EINVAL
    assert call(n=(1 << 30) + 1) in (-errno.E2BIG, EINVAL)          # so many rows reach the other buffers
    torch.cuda.synchronize()
    for t in outs:
        assert bool((t == 0xa5).all())
    assert np.array_equal(df.cpu().numpy(), f)
    # gf_forward_queues: refused before the handle's table is uploaded, the queue column untouched
    h = lib.gf_forward_load(C.byref(gf_forward_cfg(4, 0, 1, 2, 0, 0, None)))
    assert h > 0
    try:
        col = full(n)
        fq = lambda fwd=h, rec=df.data_ptr(), kind=M.REC_PIPELINE, n=8: lib.gf_forward_queues(fwd, rec, kind, n, col.data_ptr(), None)
        assert fq(fwd=987654) == -errno.EBADF and fq(rec=None) == EFAULT and fq(kind=7) == EINVAL
        assert fq(n=(1 << 30) + 1) == -errno.E2BIG and fq(n=0) == 0
        torch.cuda.synchronize()
        assert bool((col == 0xa5).all())
    finally:
        lib.gf_obj_close(h)
    # n == 0: qoff (n_queues + 1 words) and counts are zeros, nothing else is written
    assert call(n=0, fs=None, fl=None, stride=0, nq=7) == 0
    torch.cuda.synchronize()
    assert not bool(qoff[:8].any()) and bool((qoff[8:] == 0xa5).all()) and not bool(counts.any())
    for t in (snap, olen, oidx):
        assert bool((t == 0xa5).all())
    assert call() == 0                                               # and the same arguments run
    torch.cuda.synchronize()
    m = M.partition(f, ln, q, 4)
    assert Fwd.np32(qoff)[:5].tolist() == m["qoff"].tolist() and Fwd.np32(counts).tolist() == m["counts"]


# ------------------------------------------------------------------ the queue column from real records
def _classify(name):
    """(device batch, device records, snap_out) of the case's classify call on a fresh datapath."""
    from cilium_amd.datapath import Datapath, DeviceBatch
    sc, pk, rec, ifx, kind = M.case(name)
    dp = Datapath(sc, pin_prefix=None)
    b = DeviceBatch(pk, parse=False)
    if name == "pipeline":
        out, _, snap = dp.pipeline(b, sc.now)
    elif name == "egress":
        out, snap = dp.egress(b, sc.now)
    else:
        out, _, snap = dp.lb_frames(b, snap_out=True)
    torch.cuda.synchronize()
    return dp, b, out, snap


@pytest.mark.parametrize("name", ["pipeline", "egress", "lb"])
def test_queue_column_from_device_records(name):
    """gf_forward_queues over the device records of gf_pipeline_classify, gf_lxc_egress_classify and
    gf_lb_classify_frames equals the model over them, and over the oracle's records."""
    from cilium_amd.datapath import to_numpy, PIPE_OUT, EG_OUT, LB_OUT
    sc, pk, rec, ifx, kind = M.case(name)
    dp, b, out, snap = _classify(name)
    try:
        cfg = {k: v for k, v in M.CFG.items() if k != "n_queues"}
        fwd = dp.forward_load(M.CFG["n_queues"], ifindex=ifx, **cfg)
        q = dp.forward_queues(fwd, kind, out)
        torch.cuda.synchronize()
        got = q.cpu().numpy()
        dev = to_numpy(out, {"pipeline": PIPE_OUT, "egress": EG_OUT, "lb": LB_OUT}[name])
        want = M.queues(kind, dev, ifindex=ifx, **cfg)
        bad = np.nonzero(got != want)[0]
        assert not len(bad), (name, int(bad[0]), got[bad[0]], want[bad[0]], dev[bad[0]])
        if name != "lb":                                 # the oracle's records of the CPU file
            assert np.array_equal(got, M.queues(kind, rec, ifindex=ifx, **cfg)), "the oracle's records"
        assert len(np.unique(got)) >= (4 if name != "lb" else 3)
        # a second handle: every queue byte of the rule on other values, a later duplicate entry winning
        ifx2 = [(sc.host_ifindex, 0), (sc.host_ifindex, 7)]
        fwd2 = dp.forward_load(8, stack_queue=DROP, responder_queue=5, default_queue=DROP, ifindex=ifx2)
        q2 = dp.forward_queues(fwd2, kind, out).cpu().numpy()
        assert np.array_equal(q2, M.queues(kind, dev, DROP, 5, DROP, ifx2))
    finally:
        dp.close()


def test_composition_and_no_side_effects():
    """pipeline classify with snap_out -> forward_queues -> forward_frames through the Datapath
    entry points: every packed row is snap_out[index[j]], the rows of the queue of the host ifindex
    all carry action REDIRECT and that ifindex in their records, and the two forward calls leave
    the event ring's count word, its records and the stats sink as they were."""
    from cilium_amd._lib import lib
    from cilium_amd.datapath import to_numpy, PIPE_OUT
    sc, pk, rec, ifx, kind = M.case("pipeline")
    dp, b, out, snap = _classify("pipeline")
    try:
        ring = dp.set_event_ring(4096)
        stats = torch.zeros(512, dtype=torch.int64, device="cuda")
        lib.gf_set_stats_sink(C.c_void_p(stats.data_ptr()))
        try:
            out, _, snap = dp.pipeline(b, sc.now + 1)                     # fills the ring and the sink
            torch.cuda.synchronize()
            before = (ring[0].clone(), ring[1].clone(), stats.clone())
            assert int(ring[1].item()) > 0 and bool(stats.any())
            cfg = {k: v for k, v in M.CFG.items() if k != "n_queues"}
            nq = M.CFG["n_queues"]
            fwd = dp.forward_load(nq, ifindex=ifx, **cfg)
            q = dp.forward_queues(fwd, kind, out)
            rows, ln, ix, qoff, counts = dp.forward_frames(snap, b.len, q, nq)
            torch.cuda.synchronize()
            assert torch.equal(ring[0], before[0]) and torch.equal(ring[1], before[1]) and torch.equal(stats, before[2])
        finally:
            lib.gf_set_stats_sink(None)
        dev = to_numpy(out, PIPE_OUT)
        m = M.partition(snap.cpu().numpy(), b.len.cpu().numpy().view(np.uint32), q.cpu().numpy(), nq)
        k = m["counts"][0]
        assert counts.cpu().numpy().view(np.uint32).tolist() == m["counts"] and 0 < k < pk.n
        assert qoff.cpu().numpy().view(np.uint32).tolist() == m["qoff"].tolist()
        idx = ix[:k].long()
        assert np.array_equal(ix[:k].cpu().numpy().view(np.uint32), m["index"])
        assert torch.equal(rows[:k], snap[idx]) and torch.equal(ln[:k], b.len[idx])
        lo, hi = int(m["qoff"][3]), int(m["qoff"][4])                    # the host ifindex's queue
        host = dev[idx.cpu().numpy()[lo:hi]]
        assert hi - lo >= 10 and (host["action"] == M.REDIRECT).all() and (host["ifindex_lo"] == sc.host_ifindex).all()
        assert (np.diff(idx.cpu().numpy()[lo:hi]) > 0).all()             # arrival order inside the queue
        # the capacity and index options of the Python entry point
        r2, l2, i2, qo2, c2 = dp.forward_frames(snap, b.len, q, nq, max_out=10, index=False)
        torch.cuda.synchronize()
        assert i2 is None and r2.shape == (10, snap.shape[1]) and torch.equal(r2, rows[:10]) and torch.equal(qo2, qoff)
        assert c2.tolist() == [k, pk.n - k, 10, 0]
    finally:
        dp.close()
