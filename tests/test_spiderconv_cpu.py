"""CPU-side checks of the SpiderConv entry points (csrc/spider.hip): declared, bound, and their argument checks answer
before any launch -- null pointers, k > n, and shapes outside the supported ranges -- so no GPU is needed."""
import ctypes

import pytest

from scanobjectnn_amd import _lib

NAMES = ("pcops_spider_taylor_fwd", "pcops_spider_taylor_bwd", "pcops_spider_taylor_bwd_workspace_bytes",
         "pcops_spider_conv_fwd", "pcops_spider_conv_wgrad", "pcops_spider_conv_wgrad_workspace_bytes",
         "pcops_spider_conv_dgrad", "pcops_group_norm_relu_fwd", "pcops_group_norm_relu_bwd",
         "pcops_group_norm_relu_workspace_bytes")
OK, NULL, SHAPE, ARG, UNSUP = 0, -1, -2, -3, -4


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_declared_and_bound(lib):
    for name in NAMES:
        assert hasattr(lib, name)
        assert name in _lib.SIGNATURES or name in _lib.PLAIN
    assert lib.pcops_abi_version() == 4


def conv_fwd(lib, b, n, c, k, t, o):
    return lib.pcops_spider_conv_fwd(b, n, c, k, t, o, None, None, None, None, None, None, None)


@pytest.mark.parametrize("entry", ["fwd", "wgrad", "dgrad"])
def test_conv_argument_checks(lib, entry):
    def call(b, n, c, k, t, o):
        if entry == "fwd":
            return conv_fwd(lib, b, n, c, k, t, o)
        if entry == "wgrad":
            return lib.pcops_spider_conv_wgrad(b, n, c, k, t, o, None, None, None, None, None, None, None, None)
        return lib.pcops_spider_conv_dgrad(b, n, c, k, t, o, None, None, None, None, None, None, None, None)
    assert call(2, 64, 32, 20, 5, 64) == NULL            # the supported shape, no buffers
    assert call(2, 8, 32, 9, 5, 64) == ARG               # k > n
    assert call(2, 64, 32, 0, 5, 64) == ARG              # k <= 0
    assert call(2, 0, 32, 20, 5, 64) == SHAPE
    assert call(2, 64, 0, 20, 5, 64) == SHAPE
    assert call(2, 128, 32, 65, 5, 64) == UNSUP          # k > 64
    assert call(2, 64, 257, 20, 5, 64) == UNSUP          # C > 256
    assert call(2, 64, 32, 20, 5, 72) == UNSUP           # O % 16 != 0
    assert call(2, 64, 32, 20, 5, 528) == UNSUP          # O > 512
    assert call(2, 64, 32, 20, 4, 64) == UNSUP           # T != 5
    assert call(2, 64, 1, 1, 5, 16) == NULL and call(2, 64, 256, 64, 5, 512) == NULL   # range ends


def test_taylor_and_group_norm_checks(lib):
    assert lib.pcops_spider_taylor_fwd(ctypes.c_longlong(100), 5, None, None, None, None, None) == NULL
    assert lib.pcops_spider_taylor_fwd(ctypes.c_longlong(100), 3, None, None, None, None, None) == UNSUP
    assert lib.pcops_spider_taylor_fwd(ctypes.c_longlong(-1), 5, None, None, None, None, None) == SHAPE
    assert lib.pcops_spider_taylor_bwd(ctypes.c_longlong(100), 5, None, None, None, None, None, None) == NULL
    assert lib.pcops_spider_taylor_bwd_workspace_bytes(ctypes.c_longlong(100), 5) == 400
    assert lib.pcops_spider_taylor_bwd_workspace_bytes(ctypes.c_longlong(1 << 20), 5) == 256 * 400
    eps = ctypes.c_float(1e-6)
    assert lib.pcops_group_norm_relu_fwd(2, 64, 64, 16, eps, None, None, None, None, None, None, None) == NULL
    assert lib.pcops_group_norm_relu_fwd(2, 64, 64, 7, eps, None, None, None, None, None, None, None) == ARG
    assert lib.pcops_group_norm_relu_fwd(2, 64, 96, 32, eps, None, None, None, None, None, None, None) == NULL   # 3 ch
    assert lib.pcops_group_norm_relu_fwd(2, 64, 514, 2, eps, None, None, None, None, None, None, None) == UNSUP  # 257 ch
    assert lib.pcops_group_norm_relu_bwd(2, 64, 64, 16, *([None] * 11)) == NULL
    assert lib.pcops_group_norm_relu_workspace_bytes(16, 256) == 16 * 2 * 256 * 4


def test_wgrad_workspace_is_a_deterministic_split(lib):
    """the weight gradient's split-K partials: sized by the launcher's own split rule, 0 where one split fills the GPU"""
    for b, n, c, k, o in ((16, 1024, 3, 20, 32), (16, 1024, 32, 20, 64), (16, 1024, 64, 20, 128),
                          (16, 1024, 128, 20, 256)):
        nbytes = lib.pcops_spider_conv_wgrad_workspace_bytes(b, n, c, k, 5, o)
        per_split = (k * c * 5 * o + o) * 4
        assert nbytes % per_split == 0 and 0 <= nbytes // per_split <= 16
    assert lib.pcops_spider_conv_wgrad_workspace_bytes(16, 1024, 300, 20, 5, 64) == 0     # unsupported shape
    # the shapes tests/test_spider_paths_gpu.py reaches the split branches with (b, n, k, c, o -> splits): a change of the
    # split rule shows here as a diff, not as a branch that silently stops being run
    for (b, n, k, c, o), splits in (((1, 40, 5, 3, 16), 1), ((2, 64, 1, 16, 64), 2), ((3, 65, 7, 17, 48), 4),
                                    ((2, 300, 20, 40, 80), 9), ((1, 130, 20, 256, 256), 1), ((2, 520, 4, 3, 16), 16),
                                    ((1, 70, 64, 5, 32), 2), ((1, 96, 3, 256, 512), 2)):
        nbytes = lib.pcops_spider_conv_wgrad_workspace_bytes(b, n, c, k, 5, o)
        assert nbytes == (0 if splits == 1 else splits * (k * c * 5 * o + o) * 4), (b, n, k, c, o)


def test_layer_outside_the_kernel_ranges_raises_before_any_launch():
    """the native route says which shapes it takes and refuses the rest with the ranges and the switch, before it
    touches a tensor (no silent fall-back to the torch form)"""
    import torch
    from scanobjectnn_amd.spidercnn import spider_ops as S
    assert S.supported(128, 20, 5, 256, 16) and S.supported(40, 20, 5, 80, 16) and S.supported(3, 20, 5, 96, 32)
    assert not S.supported(257, 20, 5, 64, 16) and not S.supported(32, 65, 5, 64, 16)
    assert not S.supported(32, 20, 5, 72, 8) and not S.supported(32, 20, 4, 64, 16)
    z = torch.zeros
    with pytest.raises(_lib.PcopsError, match="PCOPS_SPIDER_NATIVE=0"):
        S.spider_conv(z(1, 8, 300), z(1, 8, 4, dtype=torch.int32), z(1, 8, 4, 3), z(19, 5), z(5), z(4 * 300 * 5, 64),
                      z(64), z(64), z(64), 16)
