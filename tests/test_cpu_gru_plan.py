"""The GRU layer plan (csrc/gru_layer.hpp, gru_layer_plan) through srnn_gru_layer_plan_for on
the loaded library: a pure function of (dtype, B, D, CUs, share, the two switches), so it is
checked here for a 256-CU device without one."""
import ctypes

import pytest
import torch

import samplernn_hip as H

HDR = 2048          # gx::HDR (csrc/gru_xcd.hip): header of the XCD sweeps' work area


def plan(dtype, B, D, ncu=256, share=1):
    be, fb, bb = ctypes.c_int(-1), ctypes.c_size_t(0), ctypes.c_size_t(0)
    H.lib().call('srnn_gru_layer_plan_for', dtype, B, D, ncu, share, ctypes.byref(be),
                 ctypes.byref(fb), ctypes.byref(bb))
    return H.GRU_BACKENDS[be.value], fb.value, bb.value


@pytest.fixture(autouse=True)
def _switches_default(monkeypatch):
    monkeypatch.delenv('SRNN_GRU_XCD', raising=False)
    monkeypatch.delenv('SRNN_GRU_SEQ', raising=False)


@pytest.mark.parametrize('dtype,B,D,want', [
    (H.BF16, 16, 256, 'xcd'),
    (H.BF16, 16, 128, 'seq'),       # D % 256 != 0: XCD declines
    (H.BF16, 16, 192, 'steps'),     # D % 128 != 0: both sweeps decline
    (H.F32, 16, 256, 'steps'),      # fp32 always takes steps
])
def test_plan_order(dtype, B, D, want):
    assert plan(dtype, B, D)[0] == want


def test_shared_device_chunks_xcd_and_refuses_seq(monkeypatch):
    # 256 CUs shared 8 ways: the XCD sweep chains launches of what fits 32 CUs; gru_seq's
    # 64 x 4 workgroups cannot be resident 8 times over
    assert plan(H.BF16, 128, 1024, share=8)[0] == 'xcd'
    monkeypatch.setenv('SRNN_GRU_XCD', '0')
    assert plan(H.BF16, 128, 1024, share=8)[0] == 'steps'
    assert plan(H.BF16, 128, 1024, share=1)[0] == 'seq'


def test_switches_are_read_per_call(monkeypatch):
    assert plan(H.BF16, 16, 256)[0] == 'xcd'
    monkeypatch.setenv('SRNN_GRU_XCD', '0')
    assert plan(H.BF16, 16, 256)[0] == 'seq'
    monkeypatch.setenv('SRNN_GRU_SEQ', '0')
    assert plan(H.BF16, 16, 256)[0] == 'steps'
    monkeypatch.delenv('SRNN_GRU_XCD')
    assert plan(H.BF16, 16, 256)[0] == 'xcd'


@pytest.mark.parametrize('dtype', [H.BF16, H.F32])
@pytest.mark.parametrize('B,D', [(16, 256), (16, 128), (16, 192), (128, 1024), (5, 48)])
def test_no_device_means_steps(dtype, B, D):
    assert plan(dtype, B, D, ncu=0)[0] == 'steps'


def test_work_bytes_follow_the_back_end():
    """Nonzero exactly where the chosen back end (or the driver beside it) has a work area:
    both sweeps in both directions; the steps' backward (its second dh_direct buffer, B x D
    fp32); the steps' forward only in bf16 (the bf16 copy of h0, B x D x 2)."""
    be, fb, bb = plan(H.BF16, 16, 256)
    assert be == 'xcd' and fb >= HDR and bb >= HDR and bb > fb
    be, fb, bb = plan(H.BF16, 40, 128)
    nflags = (64 * 2 + 1) * 4                      # two 32-row tiles
    assert be == 'seq' and bb == nflags
    assert fb == (nflags + 255) // 256 * 256 + 40 * 128 * 2      # + the 256-aligned h0 copy
    assert plan(H.BF16, 5, 192) == ('steps', 5 * 192 * 2, 5 * 192 * 4)
    assert plan(H.F32, 5, 48) == ('steps', 0, 5 * 48 * 4)


def test_forced_queries_answer_zero_without_a_device_or_with_the_switch_off(monkeypatch):
    # (this machine may or may not have a GPU: with the switches off the answer is 0 anyway)
    monkeypatch.setenv('SRNN_GRU_XCD', '0')
    monkeypatch.setenv('SRNN_GRU_SEQ', '0')
    assert H.gru_xcd_work_bytes(torch.bfloat16, 16, 256) == 0
    assert H.gru_xcd_bwd_work_bytes(torch.bfloat16, 16, 256) == 0
    assert H.gru_seq_supported(torch.bfloat16, 16, 128) is False
