"""libgpuflow against the recorded runs of the reference programs themselves
(tests/golden/ref_<program>_<case>.npz, see tests/test_ref_diff.py for the cases and
oracle/REFDIFF.md for the mapping).  Reads only tests/golden/."""
import numpy as np
import pytest

from oracle import ref_cases as RC
from tests import ref_diff_common as D

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(0)
    return torch


def _maps_equal(dp, fx):
    last = fx["batches"][-1]
    for name in fx["maps"]:
        assert dp.dump_map(name) == D.dump_dict(last["maps"][name]), "map %s differs from the reference" % name


@pytest.mark.parametrize("case", D.CASES)
def test_ingress_equals_reference(torch, case):
    from cilium_amd.datapath import Datapath, DeviceBatch, ING_OUT, to_numpy
    fx = D.fixture("lxc", case)
    D.check_unmodelled(fx)
    sc = RC.scenario(case)
    dp = Datapath(sc, pin_prefix=None)
    try:
        for b, pk, now in zip(fx["batches"], sc.batches, RC.nows(sc)):
            out = dp.ingress(DeviceBatch(pk), now)
            torch.cuda.synchronize()
            D.check_ingress_batch(b, pk, sc, to_numpy(out, ING_OUT))
        _maps_equal(dp, fx)
    finally:
        dp.close()


def test_ingress_batches_equals_reference(torch):
    """The hand-built case through gf_policy_ingress_classify_batches (second-stream schedule)."""
    from cilium_amd.datapath import Datapath, DeviceBatch, ING_OUT, to_numpy
    fx = D.fixture("lxc", "hand")
    sc = RC.scenario("hand")
    dp = Datapath(sc, pin_prefix=None)
    try:
        outs = dp.ingress_batches([DeviceBatch(pk) for pk in sc.batches], RC.nows(sc))
        torch.cuda.synchronize()
        for b, pk, out in zip(fx["batches"], sc.batches, outs):
            D.check_ingress_batch(b, pk, sc, to_numpy(out, ING_OUT))
        _maps_equal(dp, fx)
    finally:
        dp.close()


@pytest.mark.parametrize("case", D.CASES)
def test_lb_equals_reference(torch, case):
    from cilium_amd.datapath import Datapath, DeviceBatch, LB_OUT, to_numpy
    fx = D.fixture("lb", case)
    D.check_unmodelled(fx)
    sc = RC.scenario(case)
    dp = Datapath(sc, pin_prefix=None)
    try:
        for b, pk in zip(fx["batches"], sc.batches):
            db = DeviceBatch(pk)
            out, nd6 = dp.lb(db)
            fout, fnd6, frames = dp.lb_frames(db)
            torch.cuda.synchronize()
            rec = to_numpy(out, LB_OUT)
            assert np.array_equal(rec, to_numpy(fout, LB_OUT)) and np.array_equal(nd6.cpu().numpy(), fnd6.cpu().numpy())
            D.check_lb_batch(b, pk, rec, nd6.cpu().numpy(), frames.cpu().numpy())
    finally:
        dp.close()
