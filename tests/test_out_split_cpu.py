"""CPU: the split-output flag of the dequant GEMM entries (ASQ_EPI_OUT_SPLIT(n), n = 2 .. 4, above the association order in `epi_order` of
asq_linear_w8a8_off / asq_linear_w8a8: the N columns are n segments and segment s is its own dense [M, N / n] output) -- the flag's value, that it is a
flag and no new export, every refused argument combination (ASQ_ERR_DIM with a message), and that the orders 0 and 1 and the values refused before are
judged as before.  Every call here returns from the argument checks: no compute is launched, the pointers are never read."""
import os

import pytest
import torch

from autosmoothquant_amd import _lib as L
from autosmoothquant_amd import ops

ASQ_OK, ASQ_ERR_NULL, ASQ_ERR_DIM, ASQ_ERR_DTYPE = 0, -1, -2, -3
P = 1 << 20                     # a 16-byte aligned stand-in for every pointer
ORDERS = (L.ASQ_EPI_SCALE_FIRST, L.ASQ_EPI_ACC_FIRST)


def off(order, M, N, K, dt=1):
    return L.lib().asq_linear_w8a8_off(P, P, P, dt, M, N, K, 1.0, None, None, None, order, P, P, None)


def plain(order, M, N, K, dt=1):
    return L.lib().asq_linear_w8a8(P, P, P, dt, M, N, K, 1.0, None, None, None, order, None, 0, None)


def q8(order, M, N, K):
    return L.lib().asq_linear_w8a8_q8(P, P, P, 1, M, N, K, 1.0, None, None, None, order, 0, 0, 1.0, None, 0, None)


def test_flag_value_and_no_new_export():
    assert [L.ASQ_EPI_OUT_SPLIT(n) for n in (2, 3, 4)] == [0x200, 0x300, 0x400]
    assert L.ASQ_EPI_OUT_SPLIT(2) & 0xFF == 0 and L.ASQ_EPI_SCALE_FIRST == 0 and L.ASQ_EPI_ACC_FIRST == 1      # the order keeps the low bits
    assert L.ASQ_VERSION == 126 == L.lib().asq_version()
    assert not any("split" in name for name in L.SIGNATURES)
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "asq_hip.h")) as f:
        assert "#define ASQ_EPI_OUT_SPLIT(n) ((n) << 8)" in f.read()          # the Python mirror states the header's macro


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("entry", [off, plain], ids=["off", "plain"])
def test_refused_splits(entry, order):
    err = L.lib().asq_last_error
    for n in (1, 5, 6, 255, 1 << 10):                                       # n outside 2 .. 4
        assert entry(order | L.ASQ_EPI_OUT_SPLIT(n), 1280, 4 * 256 * n, 256) == ASQ_ERR_DIM, n
        assert b"ASQ_EPI_OUT_SPLIT" in err() and b"2 <= n <= 4" in err()
    for n, N in ((3, 4 * 256), (3, 3 * 256 + 1), (2, 2 * 256 + 1), (4, 4 * 256 + 2)):     # N % n != 0
        assert entry(order | L.ASQ_EPI_OUT_SPLIT(n), 1280, N, 256) == ASQ_ERR_DIM, (n, N)
        assert b"ASQ_EPI_OUT_SPLIT" in err()
    for n, N in ((2, 256), (2, 2 * 384), (3, 3 * 128), (4, 4 * 4600), (2, 8)):            # (N / n) % 256 != 0
        assert entry(order | L.ASQ_EPI_OUT_SPLIT(n), 1280, N, 256) == ASQ_ERR_DIM, (n, N)
        assert b"256" in err()


@pytest.mark.parametrize("order", ORDERS)
def test_int8_outputs_have_no_split_form(order):
    for n in (2, 3, 4):
        assert q8(order | L.ASQ_EPI_OUT_SPLIT(n), 1280, n * 4608, 256) == ASQ_ERR_DIM
        assert b"int8" in L.lib().asq_last_error()
    assert q8(order | L.ASQ_EPI_OUT_SPLIT(7), 1280, 7 * 256, 256) == ASQ_ERR_DIM


@pytest.mark.parametrize("order", ORDERS)
def test_shapes_off_the_256x256_class_are_refused(order):
    """asq_linear_w8a8 takes the flag only where its dispatcher runs the call on the 256 x 256 kernels"""
    name = L.lib().asq_gemm_kernel_name
    for M, Ns, K, n in ((16, 256, 256, 2),          # weight-streaming kernel
                        (512, 512, 512, 2),         # 128-row tiles
                        (1280, 512, 256, 3),        # few 256 x 256 tiles
                        (1280, 4608, 192, 3)):      # K % 128 != 0: the generic kernel
        assert name(M, n * Ns, K) != b"p16", (M, n * Ns, K)
        assert plain(order | L.ASQ_EPI_OUT_SPLIT(n), M, n * Ns, K) == ASQ_ERR_DIM, (M, Ns, K, n)
        assert b"256 x 256" in L.lib().asq_last_error()
    assert off(order | L.ASQ_EPI_OUT_SPLIT(3), 1280, 3 * 4608, 192) == ASQ_ERR_DIM      # asq_linear_w8a8_off's own shape rule comes as before


def test_orders_and_refused_values_are_judged_as_before():
    for entry in (off, plain, q8):
        for order in ORDERS:
            assert entry(order, 0, 512, 256) == ASQ_OK and entry(order, 7, 0, 256) == ASQ_OK       # an empty problem
    for entry in (plain, q8):
        for bad in (2, 3, 7, 0xFF, -1, -2, 1 << 31 - 1 | 2, -(1 << 31), L.ASQ_EPI_OUT_SPLIT(2) | 2, L.ASQ_EPI_OUT_SPLIT(3) | 0x80):
            assert entry(bad, 1280, 3 * 4608, 256) == ASQ_ERR_DTYPE, bad
            assert b"bad epi_order" in L.lib().asq_last_error()
    for bad in (2, 7, -1, L.ASQ_EPI_OUT_SPLIT(2) | 2):
        assert off(bad, 1280, 3 * 4608, 256) == ASQ_ERR_DTYPE, bad
    assert L.lib().asq_linear_w8a8_off(None, None, None, 1, 4, 4, 4, 1.0, None, None, None, L.ASQ_EPI_OUT_SPLIT(2), None, None, None) == ASQ_ERR_NULL   # pointers first


def test_ops_out_split_on_cpu_tensors_raises():
    z = lambda *s: torch.zeros(s, dtype=torch.int8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.linear_w8a8_off(z(4, 128), z(512, 128), torch.zeros(4, 2, dtype=torch.int32), torch.zeros(512, 2, dtype=torch.int32), torch.float16, out_split=2)
