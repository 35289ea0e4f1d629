"""The fused backward of the SampleLevelMLP's output layer (srnn_mlp_out_bwd, csrc/out_bwd.hip):
da2, dW_out, db_out and the hidden-bias column sums from one pass over dz and a2, against the
separate calls it replaces (masked da2 GEMM, split-K dW_out GEMM, column sum of dz) and against
fp64 products of the same bf16 operands.

Shapes (Q = 256): the smallest that exercise each mechanism -- one column slice as four
workgroups of one 128-row block and as one workgroup of two; 3 column slices with row ranges
of unequal length (3, 3 and 4 blocks); all 8 slices and the XCD map; a long accumulation chain
(128 chunks per range).
"""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda'
Q = 256
# (M, D, row ranges asked for; 0: one workgroup per CU)
CASES = [(256, 128, 0), (256, 128, 1), (1280, 384, 0), (1280, 384, 3), (8192, 1024, 0), (16384, 256, 0),
         (16384, 256, 2)]


def _inputs(M, D, q=Q):
    g = torch.Generator(device=DEV)
    g.manual_seed(1000 + M + D + q)
    dz = (torch.randn((M, q), device=DEV, generator=g) * 0.05).bfloat16()
    a2 = torch.randn((M, D), device=DEV, generator=g) * 0.5
    # ReLU output: about half the entries exactly 0, none negative
    a2 = torch.where(torch.rand((M, D), device=DEV, generator=g) < 0.5, torch.zeros_like(a2), a2)
    a2 = a2.clamp_(min=0).bfloat16()
    wt = (torch.randn((q, D), device=DEV, generator=g) * 0.03).bfloat16().t().contiguous()
    return dz, a2, wt                                   # wt = W_out^T (D, q)


@functools.lru_cache(maxsize=None)
def _case(M, D, ranges):
    """Inputs, the fused results, the separate calls' results and the fp64 references of one
    shape, computed once and shared (nothing below modifies them)."""
    import samplernn_hip as H
    dz, a2, wt = _inputs(M, D)
    fused = H.mlp_out_bwd(dz, a2, wt, ranges)
    assert fused is not None, 'shape (%d, %d) must be served' % (M, D)
    un = (H.gemm(dz, wt, transB=True, mask=a2, out_dtype=torch.bfloat16),
          H.gemm(dz, a2, transA=True), H.colsum(dz, M, Q))
    z, a, w = dz.double(), a2.double(), wt.double()
    ref_da2 = torch.where(a > 0, z @ w.t(), torch.zeros((), device=DEV, dtype=torch.float64))
    ref = (ref_da2.bfloat16(), z.t() @ a, z.sum(0))
    torch.cuda.synchronize()
    return (dz, a2, wt), fused, un, ref


def _ord(x):
    """bf16 values as integers whose order is the values' (ulp distances by subtraction)."""
    b = x.contiguous().view(torch.int16).int()
    return torch.where(b >= 0, b, -(b & 0x7fff))


@pytest.mark.parametrize('M,D,ranges', CASES)
def test_da2_matches_masked_gemm(hip, M, D, ranges):
    """(a) da2 bit for bit the masked GEMM's, atol = rtol = 0, at every shape: operands swapped
    and k ascending in one accumulator chain, the order of the pair-mode kernel and of the
    128-tile kernels that serve the shapes off the 256 x 256 path ((256, 128), (1280, 384)).
    The distances of both to the fp64 product (masked, rounded to bf16) are printed."""
    _, fused, un, ref = _case(M, D, ranges)
    r = _ord(ref[0])
    df, du = (_ord(fused[0]) - r).abs(), (_ord(un[0]) - r).abs()
    nf, nu, uf, uu = int((df > 0).sum()), int((du > 0).sum()), int(df.max()), int(du.max())
    print('da2 (%d, %d, blocks %d): vs fp64: fused %d elements off, max %d ulp; '
          'separate %d elements off, max %d ulp' % (M, D, fused[3].shape[0], nf, uf, nu, uu))
    assert torch.equal(fused[0].view(torch.int16), un[0].view(torch.int16))


@pytest.mark.parametrize('M,D,ranges', CASES)
def test_dw_out_and_db_out_error(hip, M, D, ranges):
    """(b) dW_out and db_out: fp32 sums of the same exact products as the separate calls', in
    another order -- the maximum error against the fp64 product stays within 2x the separate
    call's at the same shape, plus 1e-6 of the largest reference entry (shapes where both are
    exact)."""
    _, fused, un, ref = _case(M, D, ranges)
    for name, f, u, r in (('dW_out', fused[1], un[1], ref[1]), ('db_out', fused[2], un[2], ref[2])):
        ef = (f.double() - r).abs().max().item()
        eu = (u.double() - r).abs().max().item()
        top = r.abs().max().item()
        print('%s (%d, %d, blocks %d): max |err| fused %.3e, separate %.3e, max |ref| %.3e'
              % (name, M, D, fused[3].shape[0], ef, eu, top))
        assert ef <= 2.0 * eu + 1e-6 * top, name


@pytest.mark.parametrize('M,D,ranges', CASES)
def test_hidden_bias_partials(hip, M, D, ranges):
    """(c) the per-block column sums, reduced as mlp_backward reduces them, against the fp64
    column sum of the stored da2 (1e-4 of the largest entry)."""
    import samplernn_hip as H
    _, fused, _, _ = _case(M, D, ranges)
    csp = fused[3]
    got = H.colsum(csp, csp.shape[0], D).double()
    want = fused[0].double().sum(0)
    err, top = (got - want).abs().max().item(), want.abs().max().item()
    print('hidden bias sums (%d, %d, blocks %d): max |err| %.3e, max |ref| %.3e'
          % (M, D, csp.shape[0], err, top))
    assert err <= 1e-4 * top


@pytest.mark.parametrize('M,D,ranges', CASES)
def test_two_launches_byte_equal(hip, M, D, ranges):
    """(d) no atomics, fixed summation orders: a second launch gives the same bytes."""
    import samplernn_hip as H
    (dz, a2, wt), fused, _, _ = _case(M, D, ranges)
    again = H.mlp_out_bwd(dz, a2, wt, ranges)
    assert torch.equal(again[0].view(torch.int16), fused[0].view(torch.int16))
    for x, y in zip(again[1:], fused[1:]):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))


def _mlp_grads(B, T, D, q, fused):
    """One forward + backward of a stand-alone bf16 SampleLevelMLP: (d_upper, gradients)."""
    import model as Mo
    torch.manual_seed(5)
    mlp = Mo.SampleLevelMLP(4, D, q, False).to(DEV)
    mlp.__dict__['T'] = torch.bfloat16
    g = torch.Generator(device=DEV)
    g.manual_seed(6)
    x = torch.randint(0, q, (B, T + 3), device=DEV, generator=g)
    upper = torch.randn((B, T, D), device=DEV, generator=g) * 0.1
    dlogp = torch.randn((B, T, q), device=DEV, generator=g) * 0.01
    with torch.no_grad():
        _, ctx = Mo.mlp_forward(mlp, x, upper, mlp._param_list())
        d_upper, grads = Mo.mlp_backward(ctx, dlogp)
    torch.cuda.synchronize()
    return [d_upper] + list(grads)


@pytest.mark.parametrize('B,T,D,q', [(2, 128, 256, 128), (2, 128, 192, 256), (2, 100, 256, 256)],
                         ids=['Q128', 'D192', 'M200'])
def test_fallback_shapes_not_taken(hip, monkeypatch, B, T, D, q):
    """(e) Q = 128, D = 192 and M = 200 are reported "not taken", and mlp_backward returns
    the separate calls' gradients, byte-equal to a run with the switch off.  (Q = 128 stops
    at the entry point: the MLP's forward itself serves q_levels = 256 only -- its
    log-softmax kernel refuses anything else -- so no mlp_backward runs with it.)"""
    import model as Mo
    dz, a2, wt = _inputs(B * T, D, q)
    assert hip.mlp_out_bwd(dz, a2, wt) is None
    assert hip.lib().dll.srnn_mlp_out_bwd_ranges(hip.BF16, B * T, D, q, 0) == 0
    before = Mo._STATS['out_bwd_fused']
    monkeypatch.setenv('SRNN_OUT_BWD_FUSED', '1')
    if q != Q:
        with pytest.raises(RuntimeError, match='q_levels must be 256'):
            _mlp_grads(B, T, D, q, True)
        assert Mo._STATS['out_bwd_fused'] == before
        return
    on = _mlp_grads(B, T, D, q, True)
    assert Mo._STATS['out_bwd_fused'] == before
    monkeypatch.setenv('SRNN_OUT_BWD_FUSED', '0')
    off = _mlp_grads(B, T, D, q, False)
    assert len(on) == len(off)
    for x, y in zip(on, off):
        assert x.dtype == y.dtype and torch.equal(x, y)


def _step(batches):
    import bench
    import nn as snn
    _, pred = bench.make_model(torch.bfloat16)
    pred = pred.to(DEV)
    inp, reset, tgt, cnd, spk = batches[0]
    lp = pred(inp, reset, cnd, spk)
    loss = snn.sequence_nll_loss_bits(lp, tgt)
    loss.backward()
    torch.cuda.synchronize()
    hip_mod = __import__('samplernn_hip')
    hip_mod.check_persistent_errors()
    return float(loss.detach()), {k: p.grad.detach().float().clone()
                                  for k, p in pred.named_parameters() if p.grad is not None}


def test_step_fused_vs_separate(hip, monkeypatch):
    """(f) one configs[1]-shaped bf16 chunk at B = 16 rows with the switch on and off: the
    counter moves only with it on, and the step returns the same bits -- the loss and every
    gradient.  da2 is bit-identical ((a)); dW_out keeps the split-K GEMM's bits because the
    row ranges are its k-slices and the partials are summed by the same kernel; the hidden
    bias sums keep the da2 GEMM's epilogue order per 128-row block; db_out is the same column
    pass over dz.  (Stricter than the error bounds of (b), which hold for any range count.)"""
    import bench
    import model as Mo
    B, T, L = 16, 1024, 64
    batches = bench.gpu_batches(bench.synth_batches(B, T, L, 1, 0), DEV)
    monkeypatch.setenv('SRNN_OUT_BWD_FUSED', '1')
    n0 = Mo._STATS['out_bwd_fused']
    l_on, g_on = _step(batches)
    n1 = Mo._STATS['out_bwd_fused']
    assert n1 > n0
    monkeypatch.setenv('SRNN_OUT_BWD_FUSED', '0')
    l_off, g_off = _step(batches)
    assert Mo._STATS['out_bwd_fused'] == n1
    print('loss fused %.8f separate %.8f' % (l_on, l_off))
    assert l_on == l_off
    assert g_on.keys() == g_off.keys()
    for k in g_off:
        assert torch.equal(g_on[k], g_off[k]), k
