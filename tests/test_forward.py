"""gf_forward_load / gf_forward_queues / gf_forward_frames without a GPU: the model of
tests/forward_model.py against hand-written records for every row of the rule table of
include/gpuflow.h, the model over the oracle's records of a pipeline and an egress scenario (with
the share of every verdict class asserted), and every refusal of the three calls, which all
precede any launch (the library loads without a device; the device pointers are made-up addresses
that a refused call never follows).  The kernels are checked in tests/test_gpu_forward.py."""
import ctypes as C
import errno

import numpy as np
import pytest

from cilium_amd._lib import (lib, gf_frames, gf_forward_cfg, gf_forward_ifindex, gf_forward_out, gf_lb_cfg,
                             GF_FWD_DROP, GF_FWD_MAX_QUEUES, GF_REC_EGRESS, GF_REC_PIPELINE, GF_REC_LB)
from cilium_amd.datapath import EG_OUT, PIPE_OUT, LB_OUT
from tests import forward_model as M

EBADF, EFAULT, EINVAL, E2BIG = -errno.EBADF, -errno.EFAULT, -errno.EINVAL, -errno.E2BIG
OK, SHOT, REDIRECT = M.OK, M.SHOT, M.REDIRECT
STACK, RESP, DEFAULT = 0, 1, 2
IFX = [(3, 3), (9, 4), (11, M.DROP), (9, 5)]            # 9 twice: the later entry wins


def _recs(dt, rows):
    r = np.zeros(len(rows), dt)
    for k, row in enumerate(rows):
        for f, v in row.items():
            r[k][f] = v
    return r


# ------------------------------------------------------------------ the rule table, by hand
def test_abi_constants_and_layouts():
    assert (GF_FWD_MAX_QUEUES, GF_FWD_DROP, GF_REC_LB) == (64, 0xff, 3) == (64, M.DROP, M.REC_LB)
    assert (GF_REC_EGRESS, GF_REC_PIPELINE) == (M.REC_EGRESS, M.REC_PIPELINE)
    assert C.sizeof(gf_forward_ifindex) == 4 and C.sizeof(gf_forward_cfg) == 24 and C.sizeof(gf_forward_out) == 48
    assert gf_forward_cfg.n_ifindex.offset == 8 and gf_forward_cfg.ifindex.offset == 16
    assert gf_forward_out.max_out.offset == 24 and gf_forward_out.qoff.offset == 32
    # the record bytes k_fwd_queues reads
    assert (PIPE_OUT.fields["stage"][1], PIPE_OUT.fields["action"][1], PIPE_OUT.fields["flags"][1],
            PIPE_OUT.fields["ifindex_lo"][1]) == (0, 1, 4, 8) and PIPE_OUT.itemsize == 24
    assert (EG_OUT.fields["action"][1], EG_OUT.fields["ifindex_lo"][1], EG_OUT.fields["eg_flags"][1]) == (1, 8, 14)
    assert EG_OUT.itemsize == 24 and LB_OUT.fields["action"][1] == 0 and LB_OUT.itemsize == 12


def test_model_pipeline_records_by_hand():
    rows = [
        ({"stage": 1, "action": 1}, M.DROP),                              # 1: stage XDP (action XDP_DROP)
        ({"stage": 1, "action": OK, "flags": 0x04}, M.DROP),              #    before the responder row
        ({"stage": 3, "action": OK, "flags": 0x04, "pad0": 2}, RESP),     # 2: GF_PIPE_F_RESPONDER
        ({"stage": 3, "action": REDIRECT, "flags": 0x20, "ifindex_lo": 3}, RESP),   # GF_PIPE_F_ICMP6_TE
        ({"stage": 3, "action": SHOT, "flags": 0x20}, RESP),              #    before the action rows
        ({"stage": 2, "action": SHOT, "reason": 130}, M.DROP),            # 3
        ({"stage": 3, "action": OK}, STACK),                              # 4
        ({"stage": 4, "action": OK, "flags": 0x40 | 0x80 | 0x08 | 0x10}, STACK),   # other flag bits do not matter
        ({"stage": 4, "action": REDIRECT, "ifindex_lo": 3}, 3),           # 5: an entry
        ({"stage": 4, "action": REDIRECT, "ifindex_lo": 9}, 5),           #    the later duplicate wins
        ({"stage": 4, "action": REDIRECT, "ifindex_lo": 11}, M.DROP),     #    an entry that drops
        ({"stage": 4, "action": REDIRECT, "ifindex_lo": 12}, DEFAULT),    #    no entry
        ({"stage": 2, "action": REDIRECT, "ifindex_lo": 0}, DEFAULT),
        ({"stage": 4, "action": REDIRECT, "ifindex_lo": 65535}, DEFAULT),
        ({"stage": 4, "action": 1}, M.DROP),                              # 6: garbage action bytes
        ({"stage": 0, "action": 3}, M.DROP),
        ({"stage": 7, "action": 255, "ifindex_lo": 3}, M.DROP),
    ]
    got = M.queues(M.REC_PIPELINE, _recs(PIPE_OUT, [r for r, _ in rows]), STACK, RESP, DEFAULT, IFX)
    assert got.tolist() == [q for _, q in rows]


def test_model_egress_records_by_hand():
    rows = [
        ({"stage": 0, "action": OK, "eg_flags": 0x0800}, RESP),           # 2: GF_EG_F_ARP
        ({"stage": 0, "action": OK, "eg_flags": 0x4000 | 0x1000}, RESP),  #    GF_EG_F_RESPONDER
        ({"stage": 5, "action": REDIRECT, "eg_flags": 0x2000 | 0x1000, "ifindex_lo": 3}, RESP),   # GF_EG_F_ICMP6_TE
        ({"stage": 1, "action": SHOT, "eg_flags": 0x0800}, RESP),         #    an egress record has no stage XDP: row 1 is not taken
        ({"stage": 5, "action": SHOT, "reason": 131}, M.DROP),            # 3
        ({"stage": 5, "action": OK, "eg_flags": 0x0100}, STACK),          # 4: pass_to_stack
        ({"stage": 5, "action": REDIRECT, "eg_flags": 0x0080, "ifindex_lo": 3}, 3),    # 5: to_host
        ({"stage": 5, "action": REDIRECT, "eg_flags": 0x0040, "ifindex_lo": 9}, 5),    #    encap, the later entry
        ({"stage": 4, "action": REDIRECT, "eg_flags": 0x0200, "ifindex_lo": 21}, DEFAULT),
        ({"stage": 4, "action": REDIRECT, "flags": 0x24, "ifindex_lo": 21}, DEFAULT),  # handle_policy's flags byte is not eg_flags
        ({"stage": 5, "action": 9}, M.DROP),                              # 6
    ]
    got = M.queues(M.REC_EGRESS, _recs(EG_OUT, [r for r, _ in rows]), STACK, RESP, DEFAULT, IFX)
    assert got.tolist() == [q for _, q in rows]


def test_model_lb_records_by_hand():
    rows = [({"action": SHOT, "reason": 134}, M.DROP), ({"action": OK}, STACK), ({"action": OK, "slave": 2}, STACK),
            ({"action": REDIRECT, "slave": 1}, DEFAULT),                   # no ifindex in the record: always default_queue
            ({"action": 1}, M.DROP), ({"action": 200}, M.DROP)]
    got = M.queues(M.REC_LB, _recs(LB_OUT, [r for r, _ in rows]), STACK, RESP, DEFAULT, IFX)
    assert got.tolist() == [q for _, q in rows]
    assert M.queues(M.REC_LB, _recs(LB_OUT, [{"action": REDIRECT}]), STACK, RESP, M.DROP, IFX).tolist() == [M.DROP]


def test_model_partition_by_hand():
    frames = np.arange(8 * 14, dtype=np.uint8).reshape(8, 14)
    lens = np.arange(100, 108)
    queue = np.array([2, 0xff, 0, 2, 7, 0, 3, 2], np.uint8)               # 7 and 3: not below n_queues = 3
    p = M.partition(frames, lens, queue, 3)
    assert p["order"].tolist() == [2, 5, 0, 3, 7] and p["qoff"].tolist() == [0, 2, 2, 5]      # queue 1 is empty
    assert p["counts"] == [5, 3, 5, 2] and np.array_equal(p["snap"], frames[[2, 5, 0, 3, 7]])
    assert p["len"].tolist() == [102, 105, 100, 103, 107] and p["index"].tolist() == [2, 5, 0, 3, 7]
    p = M.partition(frames, lens, queue, 3, max_out=3)                    # the cut falls inside queue 2
    assert p["qoff"].tolist() == [0, 2, 2, 5] and p["counts"] == [5, 3, 3, 2] and p["index"].tolist() == [2, 5, 0]
    assert M.partition(frames, lens, queue, 3, snap=False)["counts"] == [5, 3, 0, 2]
    assert M.partition(frames, lens, queue, 8)["counts"] == [7, 1, 7, 0]


# ------------------------------------------------------------------ the oracle's records
@pytest.mark.parametrize("name", ["pipeline", "egress"])
def test_oracle_records_cover_every_class(name):
    """Drop, stack and redirect each hold at least 1 % of the scenario's records, from the oracle
    alone; the queue column of the model puts every record where its verdict says."""
    sc, pk, rec, ifx, kind = M.case(name)
    act = rec["action"]
    resp = (rec["eg_flags"] & M.EG_RESPONDER_FLAGS) != 0 if name == "egress" else (rec["flags"] & M.PIPE_RESPONDER_FLAGS) != 0
    xdp = rec["stage"] == M.STAGE_XDP if name == "pipeline" else np.zeros(pk.n, bool)
    share = {"drop": ((act == SHOT) | xdp).mean(), "stack": ((act == OK) & ~resp & ~xdp).mean(),
             "redirect": ((act == REDIRECT) & ~resp & ~xdp).mean()}
    assert min(share.values()) >= 0.01, share
    assert resp.sum() >= 4, "responder records"
    q = M.queues(kind, rec, ifindex=ifx, **{k: v for k, v in M.CFG.items() if k != "n_queues"})
    assert (q[xdp] == M.DROP).all() and (q[resp & ~xdp] == M.CFG["responder_queue"]).all()
    rest = ~resp & ~xdp
    assert (q[rest & (act == SHOT)] == M.DROP).all() and (q[rest & (act == OK)] == M.CFG["stack_queue"]).all()
    red = rest & (act == REDIRECT)
    host = red & (rec["ifindex_lo"] == sc.host_ifindex)
    assert host.sum() >= 10 and (q[host] == 3).all()
    other = red & ~np.isin(rec["ifindex_lo"], [i for i, _ in ifx])
    assert other.sum() >= 10 and (q[other] == M.CFG["default_queue"]).all()
    assert (q[red & (rec["ifindex_lo"] == 10)] == M.DROP).all()
    assert set(np.unique(q)) <= {0, 1, 2, 3, 4, M.DROP}
    if name == "egress":                                                  # the tunnel device: ENCAP_IFINDEX 5
        assert (red & (rec["ifindex_lo"] == 5)).sum() >= 10 and (q[red & (rec["ifindex_lo"] == 5)] == 4).all()


def test_oracle_lb_records():
    """bpf_lb's records carry no ifindex: every REDIRECT takes default_queue."""
    sc, pk, rec, ifx, kind = M.case("lb")
    act = rec["action"]
    assert min((act == SHOT).mean(), (act == OK).mean(), (act == REDIRECT).mean()) >= 0.01
    q = M.queues(kind, rec, 0, 1, 2, ifx)
    assert (q[act == REDIRECT] == 2).all() and (q[act == OK] == 0).all() and (q[act == SHOT] == M.DROP).all()


# ------------------------------------------------------------------ refusals (no device)
def _load(n_queues=4, stack=0, resp=1, default=2, ifx=((3, 3),), cfg=True, null_list=False):
    ent = (gf_forward_ifindex * max(len(ifx), 1))(*[gf_forward_ifindex(i, q, 0) for i, q in ifx])
    c = gf_forward_cfg(n_queues, stack, resp, default, 0, len(ifx), None if null_list or not len(ifx) else ent)
    return lib.gf_forward_load(C.byref(c) if cfg else None)


@pytest.fixture(scope="module")
def handles():
    h = {"fwd": _load(), "lb": lib.gf_lb_prog_load(C.byref(gf_lb_cfg(0, 0, 0, 0))), "map": lib.gf_map_create(1, 8, 8, 16, 0)}
    assert min(h.values()) > 0
    yield h
    for v in h.values():
        assert lib.gf_obj_close(v) == 0


def test_load_refusals():
    assert _load(cfg=False) == EFAULT
    assert _load(null_list=True) == EFAULT                  # n_ifindex > 0 with a NULL list
    assert _load(n_queues=0, null_list=True) == EFAULT      # -EFAULT before -EINVAL
    assert _load(n_queues=0) == EINVAL and _load(n_queues=65) == EINVAL
    for kw in ({"stack": 4}, {"resp": 4}, {"default": 0xfe}, {"ifx": ((3, 3), (4, 4))}, {"ifx": ((3, 0xfe),)}):
        assert _load(**kw) == EINVAL, kw
    for kw in ({"stack": M.DROP, "resp": M.DROP, "default": M.DROP}, {"ifx": ()}, {"ifx": ((3, M.DROP), (3, 0), (65535, 3))},
               {"n_queues": 64, "stack": 63}, {"n_queues": 1, "stack": 0, "resp": 0, "default": 0, "ifx": ((7, 0),)}):
        h = _load(**kw)
        assert h > 0, kw
        assert lib.gf_obj_close(h) == 0


def test_queues_refusals(handles):
    P = 1 << 44
    q = lambda h=handles["fwd"], rec=P, kind=GF_REC_PIPELINE, n=100, out=2 * P: lib.gf_forward_queues(h, rec, kind, n, out, None)
    for h in (0, 987654, handles["map"], handles["lb"]):
        assert q(h=h) == EBADF
    assert q(h=handles["lb"], rec=None, kind=9) == EBADF    # -EBADF first
    assert q(rec=None) == EFAULT and q(out=None) == EFAULT
    assert q(rec=None, kind=0) == EFAULT                    # -EFAULT before -EINVAL
    assert q(kind=0) == EINVAL and q(kind=4) == EINVAL
    assert q(n=(1 << 30) + 1) == E2BIG
    assert q(n=0) == 0 and q(n=0, rec=None, out=None, kind=GF_REC_LB) == 0
    assert q(n=0, kind=0) == EINVAL


class Frames:
    """gf_forward_frames over made-up device addresses; qoff and counts are host memory pre-filled
    with 0xA5 that a refused call leaves alone."""
    SNAP, LEN, QUEUE, OSNAP, OLEN, OIDX = (k << 44 for k in range(1, 7))

    def __init__(self):
        self.qoff = np.full(65, 0xa5a5a5a5, np.uint32)
        self.counts = np.full(4, 0xa5a5a5a5, np.uint32)

    def __call__(self, n=1000, stride=64, snap=SNAP, ln=LEN, queue=QUEUE, nq=4, osnap=OSNAP, olen=OLEN, oidx=OIDX,
                 max_out=1000, qoff=True, counts=True, frames=True, out=True):
        fr = gf_frames(n, stride, snap, ln)
        qo = self.qoff.ctypes.data if qoff is True else qoff
        co = self.counts.ctypes.data if counts is True else counts
        o = gf_forward_out(osnap, olen, oidx, max_out, qo or None, co or None)
        rc = lib.gf_forward_frames(C.byref(fr) if frames else None, queue, nq, C.byref(o) if out else None, None)
        assert (self.qoff == 0xa5a5a5a5).all() and (self.counts == 0xa5a5a5a5).all(), "a refused call wrote"
        return rc


def test_frames_refusals():
    f = Frames()
    assert f(frames=False) == EFAULT and f(queue=None) == EFAULT and f(out=False) == EFAULT
    assert f(qoff=None) == EFAULT and f(counts=None) == EFAULT
    assert f(snap=None) == EFAULT and f(ln=None) == EFAULT
    assert f(olen=None) == EFAULT and f(olen=None, oidx=None) == EFAULT           # out->snap without out->len
    assert f(snap=None, stride=13) == EFAULT and f(counts=None, nq=0) == EFAULT   # -EFAULT before -EINVAL
    assert f(nq=0) == EINVAL and f(nq=65) == EINVAL
    assert f(stride=13) == EINVAL and f(stride=257) == EINVAL
    assert f(osnap=None) == EINVAL and f(osnap=None, oidx=None) == EINVAL         # snap NULL with len or index
    assert f(osnap=None, olen=None) == EINVAL
    # no in-place mode: an output that shares a byte with the frames, the lengths or the queue column
    assert f(osnap=f.SNAP) == EINVAL and f(osnap=f.SNAP + 64 * 999 + 63) == EINVAL
    assert f(osnap=f.SNAP - 64 * 1000 + 1) == EINVAL
    assert f(olen=f.LEN) == EINVAL and f(oidx=f.LEN + 3999) == EINVAL
    assert f(osnap=f.QUEUE + 999) == EINVAL and f(olen=f.QUEUE) == EINVAL and f(oidx=f.QUEUE - 3999) == EINVAL
    assert f(qoff=f.QUEUE + 500) == EINVAL and f(counts=f.SNAP + 100) == EINVAL and f(qoff=f.LEN - 19) == EINVAL
    assert f(nq=64, qoff=f.QUEUE - 259) == EINVAL                                 # qoff has n_queues + 1 words
    assert f(n=(1 << 30) + 1) == E2BIG
    assert f(stride=13, n=(1 << 30) + 1) == EINVAL                                 # -EINVAL before -E2BIG
