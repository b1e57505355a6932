"""A numpy restatement of gf_forward_queues' rule table and of gf_forward_frames' stable partition
(include/gpuflow.h), the checker of tests/test_forward.py and tests/test_gpu_forward.py."""
import numpy as np

DROP = 0xff                                    # GF_FWD_DROP
REC_EGRESS, REC_PIPELINE, REC_LB = 1, 2, 3     # GF_REC_*
OK, SHOT, REDIRECT = 0, 2, 7                   # TC_ACT_*
STAGE_XDP = 1
EG_RESPONDER_FLAGS = 0x0800 | 0x4000 | 0x2000  # GF_EG_F_ARP | GF_EG_F_RESPONDER | GF_EG_F_ICMP6_TE
PIPE_RESPONDER_FLAGS = 0x20 | 0x04             # GF_PIPE_F_ICMP6_TE | GF_PIPE_F_RESPONDER


def table(default_queue, ifindex=()):
    """The 65536-entry ifindex_lo -> queue table: a later entry for the same ifindex_lo wins."""
    t = np.full(65536, default_queue, np.uint8)
    for ifx, q in ifindex:
        t[ifx] = q
    return t


def queues(kind, rec, stack_queue, responder_queue, default_queue, ifindex=()):
    """queue[i] of structured records (datapath.EG_OUT / PIPE_OUT / LB_OUT), the first rule that
    matches: stage XDP, a responder tail call pending, SHOT, OK, REDIRECT, anything else."""
    n = len(rec)
    act = rec["action"].astype(np.int64)
    xdp = np.zeros(n, bool)
    resp = np.zeros(n, bool)
    if kind == REC_EGRESS:
        resp = (rec["eg_flags"] & EG_RESPONDER_FLAGS) != 0
    elif kind == REC_PIPELINE:
        xdp = rec["stage"] == STAGE_XDP
        resp = (rec["flags"] & PIPE_RESPONDER_FLAGS) != 0
    else:
        assert kind == REC_LB
    if kind == REC_LB:
        redir = np.full(n, default_queue, np.uint8)
    else:
        redir = table(default_queue, ifindex)[rec["ifindex_lo"]]
    q = np.full(n, DROP, np.uint8)
    q[act == REDIRECT] = redir[act == REDIRECT]
    q[act == OK] = stack_queue
    q[act == SHOT] = DROP
    q[resp] = responder_queue
    q[xdp] = DROP
    return q


def partition(frames, lens, queue, n_queues, max_out=None, snap=True):
    """gf_forward_frames: a dict of order (the batch index of every forwarded row, queue-major,
    stable), qoff [n_queues + 1], counts [4], and the written prefix of snap / len / index."""
    queue = np.asarray(queue, np.uint8)
    n = len(queue)
    fwd = np.nonzero(queue < n_queues)[0]
    order = fwd[np.argsort(queue[fwd], kind="stable")]
    per = np.bincount(queue[fwd], minlength=n_queues)[:n_queues]
    qoff = np.concatenate([[0], np.cumsum(per)]).astype(np.uint32)
    cap = n if max_out is None else max_out
    w = min(len(order), cap) if snap else 0
    invalid = int(((queue >= n_queues) & (queue != DROP)).sum())
    return {"order": order, "qoff": qoff, "counts": [len(order), n - len(order), w, invalid], "written": w,
            "snap": frames[order[:w]], "len": np.asarray(lens, np.uint32)[order[:w]], "index": order[:w].astype(np.uint32)}


# ---- the scenarios both test files take their records from (computed once per process) ----
CFG = dict(n_queues=6, stack_queue=0, responder_queue=1, default_queue=2)    # plus the ifindex entries of a case
_cache = {}


def case(name):
    """(scenario, batch, oracle records, ifindex entries, rec kind) of "pipeline" (synth.pipeline_fuzz
    seed 7), "egress" (synth.egress_fuzz seed 5) or "lb" (synth.lb_frames_fuzz seed 3): 4,000 frames
    each.  The host ifindex goes to queue 3, ifindex 5 (the egress scenario's tunnel device) to
    queue 4, ifindex 10 to GF_FWD_DROP; every other redirect target takes default_queue."""
    if name not in _cache:
        from cilium_amd import synth
        from oracle.scenario import OracleDP
        if name == "pipeline":
            sc = synth.pipeline_fuzz(seed=7, n_packets=4000, n_batches=1)
            rec, kind = OracleDP(sc).pipeline(sc.batches[0], sc.now)[0], REC_PIPELINE
        elif name == "egress":
            sc = synth.egress_fuzz(seed=5, n_packets=4000, n_batches=1)
            rec, kind = OracleDP(sc).egress(sc.batches[0], sc.now)[0], REC_EGRESS
        else:
            sc = synth.lb_frames_fuzz(seed=3, n_packets=4000, n_batches=1)
            rec, kind = OracleDP(sc).lb(sc.batches[0])[0], REC_LB
        _cache[name] = (sc, sc.batches[0], rec, [(sc.host_ifindex, 3), (5, 4), (10, DROP)], kind)
    return _cache[name]
