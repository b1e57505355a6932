"""Every exported entry point that takes an object handle refuses a handle that does not exist, a
live handle of another kind, and the right handle with a null batch, with the same codes and in the
same order whichever way the library looks its handles up.  Every refusal precedes any launch, so
none of this needs a GPU: the pointers are stand-ins and are never dereferenced.

The table is what the library answers today.  Most entries answer -EBADF, -EBADF, -EFAULT; the
ones that answer otherwise say why."""
import ctypes as C
import errno

import pytest

from cilium_amd import _lib
from cilium_amd._lib import (lib, gf_xdp_cfg, gf_lb_cfg, gf_lxc_cfg, gf_netdev_cfg, gf_pipeline_cfg,
                             gf_overlay_cfg, gf_host_cfg, gf_respond_cfg, gf_tunnel_cfg, gf_event_filter_cfg)

EBADF, EFAULT, EINVAL = -errno.EBADF, -errno.EFAULT, -errno.EINVAL
MISSING = 999999
P = 0x1000                                               # a non-NULL stand-in


@pytest.fixture(scope="module")
def handles():
    """One live object of every kind, loaded without a device."""
    h = {}
    h["map"] = lib.gf_map_create(1, 8, 8, 16, 0)                           # HASH; no CT or proxy map's shape
    h["lxcmap"] = lib.gf_map_create(1, 20, 112, 16, 0)                     # cilium_lxc
    h["xdp"] = lib.gf_xdp_prog_load(C.byref(gf_xdp_cfg(0, 0, 0, 0, h["lxcmap"])))
    h["lb"] = lib.gf_lb_prog_load(C.byref(gf_lb_cfg(0, 0, 0, 0)))
    h["lxc"] = lib.gf_lxc_prog_load(C.byref(gf_lxc_cfg(lxc_id=7, seclabel=7)))
    h["array"] = lib.gf_policy_array_create()
    nd = gf_netdev_cfg(lxc_map=h["lxcmap"])
    h["pipe"] = lib.gf_pipeline_load(C.byref(gf_pipeline_cfg(0, 0, nd, h["array"])))
    h["overlay"] = lib.gf_overlay_load(C.byref(gf_overlay_cfg(h["lxcmap"], 0, 0, h["array"])))
    h["host"] = lib.gf_host_load(C.byref(gf_host_cfg(netdev=nd, policy_array=h["array"])))
    h["respond"] = lib.gf_respond_load(C.byref(gf_respond_cfg(0, 0, 0)))
    h["tunnel"] = lib.gf_tunnel_load(C.byref(gf_tunnel_cfg(mode=0, dst_port=8472, sport_min=1, sport_max=2)))
    h["filter"] = lib.gf_event_filter_load(C.byref(gf_event_filter_cfg()))
    for k, v in h.items():
        assert v > 0, (k, v)
    yield h
    for v in h.values():
        lib.gf_obj_close(v)


# (entry point, the kind of handle it wants, the call with that handle and a null batch,
#  the three answers when they are not -EBADF, -EBADF, -EFAULT)
TABLE = [
    ("gf_map_update_elem", "map", lambda h: lib.gf_map_update_elem(h, None, None, 0), None),
    ("gf_map_lookup_elem", "map", lambda h: lib.gf_map_lookup_elem(h, None, None), None),
    ("gf_map_delete_elem", "map", lambda h: lib.gf_map_delete_elem(h, None), None),
    # a null key asks for the first key; the null output is the refusal
    ("gf_map_get_next_key", "map", lambda h: lib.gf_map_get_next_key(h, None, None), None),
    ("gf_map_update_batch", "map", lambda h: lib.gf_map_update_batch(h, None, None, 4, 0, None), None),
    ("gf_map_lookup_batch", "map", lambda h: lib.gf_map_lookup_batch(h, None, None, None, None, None), None),
    ("gf_map_get_info", "map", lambda h: lib.gf_map_get_info(h, None), None),
    # pins an object of any kind; a null path is -EINVAL
    ("gf_obj_pin", "map", lambda h: lib.gf_obj_pin(h, None), (EBADF, EINVAL, EINVAL)),
    # no batch: a map of another shape than a CT map's / a proxy map's is the refusal
    ("gf_ct_gc", "map", lambda h: lib.gf_ct_gc(h, 0, None), (EBADF, EBADF, EINVAL)),
    ("gf_ct_gc_maps", "map", lambda h: lib.gf_ct_gc_maps((C.c_int * 1)(h), 1, 0, None, None), (EBADF, EBADF, EINVAL)),
    ("gf_proxy_gc", "map", lambda h: lib.gf_proxy_gc(h, 0, None), (EBADF, EBADF, EINVAL)),
    ("gf_proxy_cleanup_port", "map", lambda h: lib.gf_proxy_cleanup_port(h, 80, None), (EBADF, EBADF, EINVAL)),
    ("gf_ct_evict_log", "map", lambda h: lib.gf_ct_evict_log(h, None, 4), None),
    ("gf_xdp_classify", "xdp", lambda h: lib.gf_xdp_classify(h, None, P, None), None),
    ("gf_xdp_filter_frames", "xdp", lambda h: lib.gf_xdp_filter_frames(h, None, None, None), None),
    ("gf_lb_classify", "lb", lambda h: lib.gf_lb_classify(h, None, P, None, None), None),
    ("gf_lb_classify_frames", "lb", lambda h: lib.gf_lb_classify_frames(h, None, None, P, None, None, None), None),
    # no batch: the program was loaded without GF_LB_F_REDIRECT
    ("gf_lb_prog_set_dstmac", "lb", lambda h: lib.gf_lb_prog_set_dstmac(h, None), (EBADF, EBADF, EINVAL)),
    # no batch: a program handle that is not an endpoint program's (here: missing) is -EINVAL
    ("gf_policy_array_update", "array", lambda h: lib.gf_policy_array_update(h, 7, MISSING), (EBADF, EBADF, EINVAL)),
    ("gf_policy_ingress_classify", "array", lambda h: lib.gf_policy_ingress_classify(h, None, 1, P, None), None),
    ("gf_policy_ingress_classify_batches", "array",
     lambda h: lib.gf_policy_ingress_classify_batches(h, 1, None, None, None, None), None),
    ("gf_lxc_egress_classify", "array", lambda h: lib.gf_lxc_egress_classify(h, None, 1, P, None, None), None),
    ("gf_lxc_egress_tunnel_meta", "array",
     lambda h: lib.gf_lxc_egress_tunnel_meta(h, None, None, 4, None, None, None, None), None),
    ("gf_pipeline_classify", "pipe", lambda h: lib.gf_pipeline_classify(h, None, 1, P, None, None, None), None),
    ("gf_pipeline_classify_tunnel", "pipe",
     lambda h: lib.gf_pipeline_classify_tunnel(h, None, 1, P, None, None, None, None), None),
    ("gf_pipeline_partition", "pipe", lambda h: lib.gf_pipeline_partition(h, None, 0, 1, None, None, None, None), None),
    ("gf_overlay_classify", "overlay", lambda h: lib.gf_overlay_classify(h, None, 1, P, None, None), None),
    ("gf_overlay_classify_opts", "overlay", lambda h: lib.gf_overlay_classify_opts(h, None, None, 1, P, None, None), None),
    ("gf_host_classify", "host", lambda h: lib.gf_host_classify(h, None, 1, P, None, None), None),
    ("gf_respond", "respond", lambda h: lib.gf_respond(h, None, P, 2 * P, None), None),
    ("gf_tunnel_encap", "tunnel", lambda h: lib.gf_tunnel_encap(h, None, P, 256, P, P, None), None),
    ("gf_tunnel_decap", "tunnel", lambda h: lib.gf_tunnel_decap(h, None, None, None), None),
    ("gf_event_drain", "filter", lambda h: lib.gf_event_drain(h, None, 0, 4, 0, None, 0, None, None, None), None),
]


def test_the_table_names_exported_entry_points():
    names = [t[0] for t in TABLE]
    assert len(set(names)) == len(names)
    assert set(names) <= set(_lib.EXPORTED)


@pytest.mark.parametrize("name,kind,call,expect", TABLE, ids=[t[0] for t in TABLE])
def test_refusals_by_handle(handles, name, kind, call, expect):
    other = handles["map"] if kind == "array" else handles["array"]   # a live handle of another kind
    got = (call(MISSING), call(other), call(handles[kind]))
    assert got == (expect or (EBADF, EBADF, EFAULT)), name


def test_obj_close(handles):
    """gf_obj_close takes a handle of any kind and no batch: a second close is the missing handle."""
    m = lib.gf_map_create(1, 8, 8, 16, 0)
    assert lib.gf_obj_close(MISSING) == EBADF
    assert lib.gf_obj_close(m) == 0
    assert lib.gf_obj_close(m) == EBADF


def test_loads_refuse_handles_of_another_kind(handles):
    """The handles a load takes in its cfg: missing and of another kind are both -EBADF."""
    nd = gf_netdev_cfg(lxc_map=handles["lxcmap"])
    for bad in (MISSING, handles["map"]):
        assert lib.gf_pipeline_load(C.byref(gf_pipeline_cfg(bad, 0, nd, handles["array"]))) == EBADF
        assert lib.gf_pipeline_load(C.byref(gf_pipeline_cfg(0, bad, nd, handles["array"]))) == EBADF
        assert lib.gf_pipeline_load(C.byref(gf_pipeline_cfg(0, 0, nd, bad))) == EBADF
        assert lib.gf_overlay_load(C.byref(gf_overlay_cfg(handles["lxcmap"], 0, 0, bad))) == EBADF
        assert lib.gf_host_load(C.byref(gf_host_cfg(netdev=nd, policy_array=bad))) == EBADF
        assert lib.gf_respond_load(C.byref(gf_respond_cfg(bad, 0, 0))) == EBADF
    # cilium_lxc's shape is checked after the handle: a map, but not 20 -> 112 bytes
    nd_bad = gf_netdev_cfg(lxc_map=handles["map"])
    assert lib.gf_pipeline_load(C.byref(gf_pipeline_cfg(0, 0, nd_bad, handles["array"]))) == EINVAL
    assert lib.gf_overlay_load(C.byref(gf_overlay_cfg(handles["map"], 0, 0, handles["array"]))) == EINVAL
    assert lib.gf_host_load(C.byref(gf_host_cfg(netdev=nd_bad, policy_array=handles["array"]))) == EINVAL
    assert lib.gf_pipeline_load(C.byref(gf_pipeline_cfg(0, 0, gf_netdev_cfg(lxc_map=handles["array"]),
                                                        handles["array"]))) == EBADF
