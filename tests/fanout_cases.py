"""Operands for the ASPP fan-out (halo_fan_dwconv3x3_affine_relu_bwd_data, halo_amd.fanout.fan_depthwise_bn_relu) on top of the
cases of tests/dwmulti_cases.py: the gradients of x's further readers.  They are float32 normal draws, not the quarter steps of the
blocks' operands, so that a sum in another order rounds differently (tests/test_aspp_fanout_host.py shows it per case).  numpy only.
tests/test_aspp_fanout_host.py and tests/test_gpu_aspp_fanout.py use them."""
import numpy as np

import dwmulti_cases as K

# the cases whose g_x cannot tell ((gx_0 + gx_1) + ... + e_0) + e_1 from the extras added first: too few elements for a rounding to differ
ORDER_BLIND = ("one_pixel",)


def extras_count(name):
    """one dense and one per-plane extra; four_dilations takes a third (dense)"""
    return 3 if name == "four_dilations" else 2


def extras_for(name, m=None):
    """m (default extras_count) extras for a case: (B, C, H, W) float32 for a dense one, (B, C) for a per-plane one; the kinds
    alternate dense, per-plane, dense ..."""
    B, C, H, W, _ = K.CASES[name][0]
    rng = np.random.default_rng(7000 + list(K.CASES).index(name))
    return [rng.standard_normal((B, C, H, W) if j % 2 == 0 else (B, C)).astype(np.float32) for j in range(extras_count(name) if m is None else m)]
