"""Shared by test_conv_grid_gpu.py and test_conv_grid_net_gpu.py: the usable-CU sweep (stabnet_conv_reserve_cus) and the two tile-count
classes every persistent-grid kernel has to run in."""
import os

import pytest
import torch

U_ODD = 37                    # 3 x 37 = 111, 2 x 37 = 74, 37: G & 7 = 7, 2, 5


def cdiv(a, b):
    return -(-a // b)


@pytest.fixture
def reservation():
    """-> (cus, [(U, reserved)]): all, U_ODD and CUs / 8 usable CUs (the floor: any reserved >= CUs - CUs / 8).  The process-wide
    reservation and the tuning override are put back afterwards, also when the test fails."""
    from stabnet_amd import _lib
    L = _lib.lib()
    assert not [k for k in os.environ if k.startswith("STABNET_CONV_")], "the per-CU numbers of these tests are conv.hip's defaults"
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert cus // 8 < U_ODD < cus
    prev = L.stabnet_conv_reserve_cus(0)
    try:
        yield cus, [(cus, 0), (U_ODD, cus - U_ODD), (cus // 8, cus + 5)]
    finally:
        L.stabnet_conv_reserve_cus(prev)
        L.stabnet_conv_tuning_override(-1, -1)


def check_tile_classes(cls, T, per_cu, us, what=""):
    """Class "a": G < T < 2G (some workgroups two tiles, the rest one).  Class "b": T >= 3G + 1, T % G != 0.  With G = per_cu x U at
    every U of `us` (the reduced grids) -> [(U, T, G)]."""
    table = []
    for U in us:
        G = per_cu * U
        if cls == "a":
            assert G < T < 2 * G, (what, U, T, G)
        else:
            assert cls == "b" and T >= 3 * G + 1 and T % G != 0, (what, U, T, G)
        table.append((U, T, G))
    assert (per_cu * U_ODD) & 7 != 0
    return table


def launched_kernel(L):
    """Name of the conv kernel this thread launched last (the launch's own route)."""
    return L.stabnet_prof_kind_name(L.stabnet_conv_last_launch_kind()).decode()
