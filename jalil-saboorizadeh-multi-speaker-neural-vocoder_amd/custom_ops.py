"""torch.library registration of the HIP operators ("registered as torch.library
custom ops, wrapped by the new model.py classes").

The drop-in classes call these ops, so the registered ops ARE the product path:

  srnn::tier_fwd / tier_bwd     FrameLevelRNN.forward (model.py:180-263) and its backward:
                                input / cond / speaker projections, the GRU sweep(s),
                                LearnedUpsampling1d -- model.tier_forward / tier_backward
  srnn::mlp_fwd / mlp_bwd       SampleLevelMLP.forward (model.py:308-325) + log_softmax
  srnn::nll_bits / nll_bits_bwd sequence_nll_loss_bits (nn.py:66-70); its backward hands the
                                MLP the gradient in closed form (fused NLL + log-softmax)
  srnn::upsample / upsample_bwd LearnedUpsampling1d used on its own (nn.py:7-43)
  srnn::dequant                 2 * udequantize / linear_dequantize (utils.py:18-19, 62-63)
  srnn::adam_clip_              gradient_clipping + Adam (optim.py:4-21), in place
  srnn::step_advance_           the device step counters srnn::adam_clip_ can read (graph mode)
  srnn::generate                Generator.__call__'s sample loop (model.py:445-520)
  srnn::generate_ctrl           the same loop with per-row temperature / top-k in the draw
  srnn::generate_ctrl_p         ... and a per-row nucleus (top-p) cut-off
  srnn::generate_stream         the loop over a chunk of a stream: carried state in / out, a
                                Philox step origin, a forced prefix; optional controls
  srnn::sample_rows             the loops' row sampler on caller-chosen logits
  srnn::generate_scored         srnn::generate_rows that also returns every step's score pair
                                (log-prob of the step's sample, entropy of the softmax)
  srnn::sample_rows_scored      srnn::sample_rows with the rows' score pairs
  srnn::gen_session_chunk_scored  a chunk of a session opened for scores, with its score pairs
  srnn::gen_session_chunk       one chunk of a generation session (model.GenSession): the loop
                                from the session's kept weights, workspace, records and graph
  srnn::gen_session_state       the session's records
(gen_session_open / _replace / _stats / _close are plain functions: they return or take the
session's handle and no tensor comes back)

Every op has a fake (meta) kernel, so FakeTensor / torch.compile tracing sees shapes without
running HIP code, and the differentiable ones have their autograd formula attached with
torch.library.register_autograd (backward = the *_bwd op).

Saved activations: a forward op returns, beside its outputs, a 0-element int64 host `handle`;
the activations its backward needs (bf16 operand copies, GRU gates, MLP a1 / a2 / log-probs)
stay in a per-call stash keyed by that handle and are released with the handle (when autograd
frees the graph, or at once under no_grad).  The backward op takes the handle.  This keeps the
forward outputs free of aliasing with inputs (custom ops may not return views of their inputs,
and many saved tensors are the fp32 parameters themselves in the fp32 mode) without copying.
"""
import weakref
from typing import Optional

import torch
from torch import Tensor

import samplernn_hip as H

_STASH = {}
_NEXT = [1]


def _stash(state):
    """A 0-element int64 host tensor standing for `state` (its key rides as an attribute of
    the tensor object, so the handle has no data: equal across runs for every comparison)."""
    key = _NEXT[0]
    _NEXT[0] += 1
    _STASH[key] = state
    handle = torch.empty(0, dtype=torch.int64)
    handle._srnn_key = key
    weakref.finalize(handle, _STASH.pop, key, None)
    return handle


def _take(handle):
    st = _STASH.get(getattr(handle, '_srnn_key', None))
    if st is None:
        raise RuntimeError('srnn: saved state of this forward is gone (backward run twice '
                           'without retain_graph, or the handle was dropped)')
    return st


def _empty():
    return torch.empty(0)


def _opt(t):
    return None if t is None or t.numel() == 0 else t


# ------------------------------------------------------------------ FrameLevelRNN
@torch.library.custom_op('srnn::tier_fwd', mutates_args=())
def tier_fwd(prev: Tensor, upper: Optional[Tensor], cond: Optional[Tensor],
             spk: Optional[Tensor], hidden: Optional[Tensor], h0: Tensor, params: list[Tensor],
             meta: list[int]) -> tuple[Tensor, Tensor, Tensor]:
    import model
    spec = model.TierSpec(meta, params)
    y, h_new, st = model.tier_forward(spec, prev, upper, cond, spk, hidden, h0, params)
    return y, h_new, _stash(st)


@tier_fwd.register_fake
def _(prev, upper, cond, spk, hidden, h0, params, meta):
    B, Fr, _ = prev.shape
    D, k, L, feeds, dt = meta[0], meta[2], meta[3], meta[5], meta[6]
    ydt = torch.bfloat16 if (feeds and dt) else torch.float32
    return (prev.new_empty((B, Fr * k, D), dtype=ydt),
            prev.new_empty((L, B, D), dtype=torch.float32),
            torch.empty(0, dtype=torch.int64, device='cpu'))


@torch.library.custom_op('srnn::tier_bwd', mutates_args=())
def tier_bwd(dy: Tensor, handle: Tensor, params: list[Tensor], meta: list[int], need_h0: bool,
             has_upper: bool) -> list[Tensor]:
    """[d_upper (B, F, D) fp32 | empty, dh0 (n_rnn, D) | empty, *parameter gradients
    (_param_list order)]."""
    import model
    d_upper, dh0, grads = model.tier_backward(_take(handle), dy, need_h0)
    return [d_upper if has_upper else _empty().to(dy.device),
            dh0 if need_h0 else _empty().to(dy.device)] + list(grads)


@tier_bwd.register_fake
def _(dy, handle, params, meta, need_h0, has_upper):
    B, FK, D = dy.shape
    k, L = meta[2], meta[3]
    return [dy.new_empty((B, FK // k, D), dtype=torch.float32) if has_upper else dy.new_empty(0),
            dy.new_empty((L, D), dtype=torch.float32) if need_h0 else dy.new_empty(0)] + \
        [torch.empty_like(p) for p in params]


def _tier_setup(ctx, inputs, output):
    prev, upper, cond, spk, hidden, h0, params, meta = inputs
    ctx.has_upper = upper is not None
    ctx.need_h0 = hidden is None and h0.requires_grad
    ctx.nparams = len(params)
    ctx.params = params
    ctx.meta = meta
    ctx.save_for_backward(output[2])
    ctx.mark_non_differentiable(output[1], output[2])


def _tier_backward(ctx, dy, dh_new, dhandle):
    (handle,) = ctx.saved_tensors
    out = torch.ops.srnn.tier_bwd(dy.contiguous(), handle, ctx.params, ctx.meta, ctx.need_h0,
                                  ctx.has_upper)
    d_upper = out[0] if ctx.has_upper else None
    dh0 = out[1] if ctx.need_h0 else None
    return None, d_upper, None, None, None, dh0, list(out[2:]), None


tier_fwd.register_autograd(_tier_backward, setup_context=_tier_setup)


def tier(prev, upper, cond, spk, hidden, h0, params, meta):
    """(conditioning for the tier below (B, F * k, D), new hidden (n_rnn, B, D))."""
    y, h_new, _ = torch.ops.srnn.tier_fwd(prev, upper, cond, spk, hidden, h0, params, meta)
    return y, h_new


# ------------------------------------------------------------------ SampleLevelMLP
@torch.library.custom_op('srnn::mlp_fwd', mutates_args=())
def mlp_fwd(x: Tensor, upper: Tensor, params: list[Tensor],
            meta: list[int]) -> tuple[Tensor, Tensor]:
    import model
    logp, st = model.mlp_forward(model.MlpSpec(meta, params), x, upper, params)
    return logp, _stash(st)


@mlp_fwd.register_fake
def _(x, upper, params, meta):
    B, Tl, _ = upper.shape
    return (upper.new_empty((B, Tl, meta[0]), dtype=torch.float32),
            torch.empty(0, dtype=torch.int64, device='cpu'))


@torch.library.custom_op('srnn::mlp_bwd', mutates_args=())
def mlp_bwd(dlogp: Tensor, handle: Tensor, params: list[Tensor], meta: list[int],
            upper_bf16: bool, nll_target: Optional[Tensor], nll_scale: float,
            nll_g: Optional[Tensor]) -> list[Tensor]:
    """[d_upper, *parameter gradients].  nll_target given: the log-probs' gradient is
    sequence_nll_loss_bits' closed form -nll_scale * nll_g * onehot(target) (dlogp unread)."""
    import model
    nll = None
    if nll_target is not None:
        nll = (nll_target, nll_target.shape[1], nll_scale, nll_g)
    d_upper, grads = model.mlp_backward(_take(handle), dlogp, nll)
    return [d_upper] + list(grads)


@mlp_bwd.register_fake
def _(dlogp, handle, params, meta, upper_bf16, nll_target, nll_scale, nll_g):
    B, Tl, _ = dlogp.shape
    udt = torch.bfloat16 if upper_bf16 else torch.float32
    return [dlogp.new_empty((B, Tl, meta[1]), dtype=udt)] + [torch.empty_like(p) for p in params]


class FusedNllToken:
    """Marks the MLP's log-prob output so the NLL backward can hand the MLP its loss gradient
    in closed form instead of a dense (B, T, Q) fp32 tensor; `emitted` records that it did,
    so the MLP backward can refuse a placeholder that autograd summed with another gradient
    (log-probs used twice) instead of computing a wrong result."""
    __slots__ = ('emitted',)

    def __init__(self):
        self.emitted = False


def _mlp_setup(ctx, inputs, output):
    x, upper, params, meta = inputs
    ctx.params = params
    ctx.meta = meta
    ctx.upper_bf16 = upper.dtype == torch.bfloat16
    ctx.save_for_backward(output[1])
    ctx.mark_non_differentiable(output[1])
    ctx.tok = FusedNllToken()
    output[0]._srnn_nll_token = ctx.tok


def _mlp_backward(ctx, dlogp, dhandle):
    (handle,) = ctx.saved_tensors
    nll = getattr(dlogp, '_srnn_nll', None)
    if nll is None and ctx.tok.emitted:
        raise RuntimeError('the fused NLL gradient of the MLP log-probs was combined with '
                           'another gradient (log-probs used twice); run with SRNN_FUSED_NLL=0')
    if nll is not None:
        out = torch.ops.srnn.mlp_bwd(dlogp, handle, ctx.params, ctx.meta, ctx.upper_bf16,
                                     nll[0], nll[1], nll[2])
    else:
        out = torch.ops.srnn.mlp_bwd(dlogp, handle, ctx.params, ctx.meta, ctx.upper_bf16, None,
                                     0.0, None)
    return None, out[0], list(out[1:]), None


mlp_fwd.register_autograd(_mlp_backward, setup_context=_mlp_setup)


def mlp(x, upper, params, meta):
    logp, _ = torch.ops.srnn.mlp_fwd(x, upper, params, meta)
    return logp


# ------------------------------------------------------------------ NLL in bits
@torch.library.custom_op('srnn::nll_bits', mutates_args=())
def nll_bits(logp: Tensor, target: Tensor) -> Tensor:
    import nn
    B, T, Q = logp.shape
    lp = logp.contiguous()
    tg = target.reshape(B, T).contiguous()
    rows = torch.empty(B * T, device=lp.device, dtype=torch.float32)
    H.lib().call('srnn_nll_fwd', H.ptr(lp), Q, H.ptr(tg), T, T, B * T, H.ptr(rows), H.stream())
    return H.colsum(rows, B * T, 1, alpha=nn.LOG2E / (B * T)).reshape(())


@nll_bits.register_fake
def _(logp, target):
    return logp.new_empty((), dtype=torch.float32)


@torch.library.custom_op('srnn::nll_bits_bwd', mutates_args=())
def nll_bits_bwd(g: Tensor, target: Tensor, B: int, T: int, Q: int, dense: bool) -> Tensor:
    """dense: the (B, T, Q) fp32 gradient -g log2(e)/N onehot(target); else a zero
    placeholder (the MLP consumes the closed form, mlp_bwd's nll_* arguments)."""
    import nn
    if not dense:
        return torch.zeros((), device=target.device, dtype=torch.float32).expand(B, T, Q)
    tg = target.reshape(B, T).contiguous()
    gd = g.detach().float().reshape(1).contiguous()
    d = torch.empty((B, T, Q), device=tg.device, dtype=torch.float32)
    H.lib().call('srnn_nll_bwd', H.ptr(tg), T, T, B * T, Q, H.ptr(d), Q, nn.LOG2E / (B * T),
                 H.ptr(gd), H.stream())
    return d


@nll_bits_bwd.register_fake
def _(g, target, B, T, Q, dense):
    return target.new_empty((B, T, Q), dtype=torch.float32)


def _nll_setup(ctx, inputs, output):
    logp, target = inputs
    ctx.shape = tuple(logp.shape)
    ctx.save_for_backward(target)
    import nn
    tok = getattr(logp, '_srnn_nll_token', None)
    # (the closed-form hand-over relies on Python attributes travelling with the gradient:
    #  eager autograd only, never while a compiler traces the backward)
    ctx.tok = tok if (nn.FUSED_NLL and isinstance(tok, FusedNllToken) and ctx.shape[2] == 256
                      and not torch.compiler.is_compiling()) else None


def _nll_backward(ctx, g):
    import nn
    (target,) = ctx.saved_tensors
    B, T, Q = ctx.shape
    d = torch.ops.srnn.nll_bits_bwd(g, target, B, T, Q, ctx.tok is None)
    if ctx.tok is not None:
        tg = target.reshape(B, T).contiguous()
        d._srnn_nll = (tg, nn.LOG2E / (B * T), g.detach().float().reshape(1).contiguous())
        ctx.tok.emitted = True
    return d, None


nll_bits.register_autograd(_nll_backward, setup_context=_nll_setup)


# ------------------------------------------------------------------ LearnedUpsampling1d
@torch.library.custom_op('srnn::upsample', mutates_args=())
def upsample(x: Tensor, params: list[Tensor], k: int, weight_norm: bool,
             has_bias: bool) -> tuple[Tensor, Tensor]:
    import nn
    out, st = nn.upsample_forward(x, params, k, weight_norm, has_bias)
    return out, _stash(st)


@upsample.register_fake
def _(x, params, k, weight_norm, has_bias):
    B, Cin, Lx = x.shape
    v = params[1] if weight_norm else params[0]
    return (x.new_empty((B, v.shape[1], Lx * k), dtype=torch.float32),
            torch.empty(0, dtype=torch.int64, device='cpu'))


@torch.library.custom_op('srnn::upsample_bwd', mutates_args=())
def upsample_bwd(dout: Tensor, handle: Tensor, params: list[Tensor], k: int,
                 weight_norm: bool) -> list[Tensor]:
    import nn
    dx, grads = nn.upsample_backward(_take(handle), dout)
    return [dx] + list(grads)


@upsample_bwd.register_fake
def _(dout, handle, params, k, weight_norm):
    B, _, LK = dout.shape
    cin = (params[1] if weight_norm else params[0]).shape[0]
    return [dout.new_empty((B, cin, LK // k), dtype=torch.float32)] + \
        [torch.empty_like(p) for p in params]


def _up_setup(ctx, inputs, output):
    ctx.params = inputs[1]
    ctx.k, ctx.wn = inputs[2], inputs[3]
    ctx.save_for_backward(output[1])
    ctx.mark_non_differentiable(output[1])


def _up_backward(ctx, dout, dhandle):
    (handle,) = ctx.saved_tensors
    out = torch.ops.srnn.upsample_bwd(dout.contiguous(), handle, ctx.params, ctx.k, ctx.wn)
    return out[0], list(out[1:]), None, None, None


upsample.register_autograd(_up_backward, setup_context=_up_setup)


# ------------------------------------------------------------------ mu-law dequantisation
@torch.library.custom_op('srnn::dequant', mutates_args=())
def dequant(samples: Tensor, q_levels: int, scale: float, mode: int) -> Tensor:
    """scale * (udequantize (mode 0) | linear_dequantize (mode 1)) of int64 indices."""
    import utils
    return utils._dequant_impl(samples, q_levels, scale, mode)


@dequant.register_fake
def _(samples, q_levels, scale, mode):
    return samples.new_empty(samples.shape, dtype=torch.float32)


# ------------------------------------------------------------------ clip + Adam
@torch.library.custom_op('srnn::adam_clip_',
                         mutates_args=('params', 'grads', 'exp_avg', 'exp_avg_sq', 'shadows'))
def adam_clip_(params: list[Tensor], grads: list[Optional[Tensor]], exp_avg: list[Tensor],
               exp_avg_sq: list[Tensor], shadows: list[Optional[Tensor]], grad_scale: float,
               clip_lo: float, clip_hi: float, lr: float, beta1: float, beta2: float,
               eps: float, step: int, dstep: Optional[Tensor] = None) -> None:
    """gradient_clipping(lo, hi) + torch.optim.Adam over every tensor in ONE launch per 64
    (srnn_adam_clip_multi3): g = clamp(g * grad_scale) (written back for fp32 gradients),
    moments and parameters updated in place, bf16 shadows (optional) refreshed; a None
    gradient is an all-zero one; skipped on the device while the persistent-sweep failure
    flag is up.  All gradients share one dtype (fp32, or bf16 from DP buckets).  dstep: a
    one-element int64 device tensor holding the count of completed steps, read by the
    kernel in place of `step` (a graph-replayed step; advanced by srnn::step_advance_)."""
    import ctypes
    n = len(params)
    if n == 0:
        return
    if dstep is not None and (dstep.dtype != torch.int64 or dstep.numel() < 1 or
                              dstep.device != params[0].device):
        raise ValueError('adam_clip_: dstep must be an int64 tensor on the parameters\' device')
    arr = lambda ts: (ctypes.c_void_p * n)(*[H.ptr(t) for t in ts])  # noqa: E731
    gdt = next((g.dtype for g in grads if g is not None), torch.float32)
    H.lib().call('srnn_adam_clip_multi3', n, arr(params), arr(grads), H.dcode(gdt),
                 float(grad_scale), arr(exp_avg), arr(exp_avg_sq),
                 arr(shadows) if any(t is not None for t in shadows) else None,
                 (ctypes.c_int64 * n)(*[p.numel() for p in params]), float(clip_lo),
                 float(clip_hi), float(lr), float(beta1), float(beta2), float(eps), int(step),
                 H.ptr(dstep) if dstep is not None else None, H.stream())


@adam_clip_.register_fake
def _(params, grads, exp_avg, exp_avg_sq, shadows, grad_scale, clip_lo, clip_hi, lr, beta1,
      beta2, eps, step, dstep=None):
    return None


@torch.library.custom_op('srnn::step_advance_', mutates_args=('dstep',))
def step_advance_(dstep: Tensor) -> None:
    """Device step counters += 1 unless the persistent-sweep failure flag is up
    (srnn_step_advance): the count srnn::adam_clip_ reads when given dstep."""
    if dstep.dtype != torch.int64 or not dstep.is_contiguous():
        raise ValueError('step_advance_: contiguous int64 counters')
    H.lib().call('srnn_step_advance', H.ptr(dstep), dstep.numel(), H.stream())


@step_advance_.register_fake
def _(dstep):
    return None


# ------------------------------------------------------------------ generation
def _generate(weights, meta, cond, row_bias, noise, seed, row_offset, flags, return_logp,
              temperature=None, top_k=None, top_p=None, state=None, step0=0, prefix=None,
              n_forced=None, return_state=False, noise_row=None, row_step0=None,
              return_scores=False):
    """The one path into the library's generation (srnn_generate6; srnn_generate7 with
    return_scores), behind the registered ops, which check their arguments first: allocates seq
    (q_zero history, the prefix written in), logp, the end state and the workspace, fills
    SrnnGenStream and SrnnGenRows and calls.  Everything at its default launches the plain
    kernels.  Returns (seq, logp, end state or empty), with return_scores also the (T, n_seqs,
    2) score pairs."""
    import ctypes
    import model
    m = model.srnn_model_struct(weights, meta)
    n_seqs, num_cond = cond.shape[0], cond.shape[1]
    L = m.tier[m.n_tiers - 1].n_frame_samples
    T = num_cond * L
    Q = m.q_levels
    dev = cond.device
    seq = torch.full((n_seqs, L + T), Q // 2, dtype=torch.long, device=dev)   # q_zero
    if prefix is not None:
        seq[:, L:L + prefix.shape[1]] = prefix.clamp(0, Q - 1)
    logp = torch.empty((T, n_seqs, Q), device=dev) if return_logp else torch.empty(0, device=dev)
    st = H.SrnnGenStream()
    st.step0 = int(step0)
    st.n_forced = H.ptr(n_forced)
    row_bytes = int(H.lib().dll.srnn_gen_state_bytes(ctypes.byref(m), 1)) if return_state else 0
    out_state = torch.empty((n_seqs, row_bytes) if return_state else (0,), dtype=torch.uint8,
                            device=dev)
    if return_state:
        st.state_out = H.ptr(out_state)
        st.state_bytes = out_state.numel()
    if state is not None:
        st.state_in = H.ptr(state)
        st.state_bytes = state.numel()
    sz = ctypes.c_size_t(0)
    H.lib().call('srnn_gen_workspace_size', ctypes.byref(m), n_seqs, ctypes.byref(sz))
    ws = torch.empty(sz.value, device=dev, dtype=torch.uint8)
    rows = H.SrnnGenRows(H.ptr(noise_row), H.ptr(row_step0))
    args = (ctypes.byref(m), n_seqs, num_cond, H.ptr(cond),
            H.ptr(row_bias), H.ptr(noise), int(seed) & ((1 << 64) - 1), int(row_offset),
            H.ptr(seq), H.ptr(logp) if return_logp else None, H.ptr(ws), sz.value, int(flags),
            H.stream(), H.ptr(temperature), H.ptr(top_k), H.ptr(top_p), ctypes.byref(st),
            ctypes.byref(rows) if noise_row is not None or row_step0 is not None else None)
    if return_scores:
        score = torch.empty((T, n_seqs, 2), device=dev)
        H.lib().call('srnn_generate7', *args, H.ptr(score))
        return seq, logp, out_state, score
    H.lib().call('srnn_generate6', *args)
    return seq, logp, out_state


def _generate_fake(meta, cond, return_logp):
    n_seqs, num_cond = cond.shape[0], cond.shape[1]
    L = meta[-1]
    Q = meta[3]                      # q_levels (model.generation_weights' meta layout)
    T = num_cond * L
    return (cond.new_empty((n_seqs, L + T), dtype=torch.long),
            cond.new_empty((T, n_seqs, Q) if return_logp else (0,)))


@torch.library.custom_op('srnn::generate', mutates_args=())
def generate(weights: list[Tensor], meta: list[int], cond: Tensor, row_bias: Tensor,
             noise: Optional[Tensor], seed: int, row_offset: int, flags: int,
             return_logp: bool) -> tuple[Tensor, Tensor]:
    """The whole autoregressive loop (model.py:445-520) on the device: (sample indices
    (n_seqs, L + T) int64, per-step log-probs (T, n_seqs, Q) or empty).  weights / meta:
    model.generation_weights' tensors and layout."""
    return _generate(weights, meta, cond, row_bias, noise, seed, row_offset, flags,
                     return_logp)[:2]


@generate.register_fake
def _(weights, meta, cond, row_bias, noise, seed, row_offset, flags, return_logp):
    return _generate_fake(meta, cond, return_logp)


def _check_rows(op, n_seqs, dev, *arrays):
    for name, t, dt in arrays:
        if (t.dtype != dt or t.dim() != 1 or t.shape[0] != n_seqs or not t.is_contiguous() or
                t.device != dev):
            raise ValueError('%s: %s must be a contiguous (%d,) %s tensor on %s'
                             % (op, name, n_seqs, dt, dev))


@torch.library.custom_op('srnn::generate_ctrl', mutates_args=())
def generate_ctrl(weights: list[Tensor], meta: list[int], cond: Tensor, row_bias: Tensor,
                  noise: Optional[Tensor], seed: int, row_offset: int, flags: int,
                  return_logp: bool, temperature: Tensor, top_k: Tensor) -> tuple[Tensor, Tensor]:
    """srnn::generate with per-row sampling controls in the draw (srnn_generate3):
    temperature (n_seqs,) float32, finite and >= 0 (0 = greedy); top_k (n_seqs,) int32 in
    [0, Q] (0 and Q = off).  model.sampling_controls validates and builds both.  The returned
    log-probs stay the model's own log-softmax, not the tempered / truncated distribution."""
    _check_rows('generate_ctrl', cond.shape[0], cond.device,
                ('temperature', temperature, torch.float32), ('top_k', top_k, torch.int32))
    return _generate(weights, meta, cond, row_bias, noise, seed, row_offset, flags, return_logp,
                     temperature, top_k)[:2]


@generate_ctrl.register_fake
def _(weights, meta, cond, row_bias, noise, seed, row_offset, flags, return_logp, temperature,
      top_k):
    return _generate_fake(meta, cond, return_logp)


@torch.library.custom_op('srnn::generate_ctrl_p', mutates_args=())
def generate_ctrl_p(weights: list[Tensor], meta: list[int], cond: Tensor, row_bias: Tensor,
                    noise: Optional[Tensor], seed: int, row_offset: int, flags: int,
                    return_logp: bool, temperature: Tensor, top_k: Tensor,
                    top_p: Tensor) -> tuple[Tensor, Tensor]:
    """srnn::generate_ctrl with the rows' nucleus mass as well (srnn_generate4): top_p (n_seqs,)
    float32 in (0, 1] (1 = off), which model.nucleus_control validates and builds.  The draw is
    then taken over the smallest set of most probable classes of the top-k set whose tempered
    mass reaches top_p (the crossing class included, ties kept)."""
    _check_rows('generate_ctrl_p', cond.shape[0], cond.device,
                ('temperature', temperature, torch.float32), ('top_k', top_k, torch.int32),
                ('top_p', top_p, torch.float32))
    return _generate(weights, meta, cond, row_bias, noise, seed, row_offset, flags, return_logp,
                     temperature, top_k, top_p)[:2]


@generate_ctrl_p.register_fake
def _(weights, meta, cond, row_bias, noise, seed, row_offset, flags, return_logp, temperature,
      top_k, top_p):
    return _generate_fake(meta, cond, return_logp)


def gen_state_row_bytes(meta):
    """Bytes of one row's record of the carried generation state (srnn_gen_state_bytes) for
    model.generation_weights' meta, under the process's fold switches.  Reads the layout
    integers only, so it also serves the fake registration."""
    import ctypes
    m = H.SrnnModel()
    m.n_tiers, m.n_rnn, m.dim, m.q_levels, m.cond_dim, m.dtype = [int(v) for v in meta[:6]]
    for k in range(m.n_tiers):
        t = m.tier[k]
        t.frame_size, t.n_frame_samples, t.in_dim, _ = [int(v) for v in meta[6 + 4 * k: 10 + 4 * k]]
        t.b_up = 1               # (generation_weights always supplies the upsampling bias)
    n = int(H.lib().dll.srnn_gen_state_bytes(ctypes.byref(m), 1))
    if n <= 0:
        raise ValueError('generate_stream: no state layout for this model')
    return n


@torch.library.custom_op('srnn::generate_stream', mutates_args=())
def generate_stream(weights: list[Tensor], meta: list[int], cond: Tensor, row_bias: Tensor,
                    noise: Optional[Tensor], seed: int, row_offset: int, flags: int,
                    return_logp: bool, temperature: Optional[Tensor], top_k: Optional[Tensor],
                    top_p: Optional[Tensor], state: Optional[Tensor], step0: int,
                    prefix: Optional[Tensor], prefix_len: Optional[Tensor],
                    return_state: bool) -> tuple[Tensor, Tensor, Tensor]:
    """srnn::generate_ctrl_p over a chunk of a stream (srnn_generate5): every control is
    optional (None = its default; all None: the plain kernels of srnn::generate), and
      state       (n_seqs, row_bytes) uint8 records of an earlier call's end state to continue
                  from, or None for a fresh start (h0, q_zero history)
      step0       generation steps the stream completed before this call: the origin of the
                  Philox counters (a replayed `noise` stays indexed from the call's first step)
      prefix      (n_seqs, P) int64 sample indices, P <= T, or None; values are clamped to
                  [0, Q)
      prefix_len  (n_seqs,) int32 in [0, P]: row b's first prefix_len[b] steps take
                  prefix[b] in place of the draw (log-probs and noise consumption unchanged);
                  None = P for every row
      return_state  also return the state the call ends in, else an empty tensor
    Returns (seq (n_seqs, L + T) int64, logp (T, n_seqs, Q) or empty, state)."""
    return _generate_stream('generate_stream', weights, meta, cond, row_bias, noise, seed,
                            row_offset, flags, return_logp, temperature, top_k, top_p, state, step0,
                            prefix, prefix_len, return_state)


def _generate_stream(op, weights, meta, cond, row_bias, noise, seed, row_offset, flags,
                     return_logp, temperature, top_k, top_p, state, step0, prefix, prefix_len,
                     return_state, noise_row=None, row_step0=None, return_scores=False):
    """The argument checks and the call of srnn::generate_stream, srnn::generate_rows and
    srnn::generate_scored."""
    n_seqs, dev = cond.shape[0], cond.device
    T = cond.shape[1] * meta[-1]            # steps of the call (meta: _generate_fake)
    ctl = [(n, t, dt) for n, t, dt in (('temperature', temperature, torch.float32),
                                       ('top_k', top_k, torch.int32),
                                       ('top_p', top_p, torch.float32)) if t is not None]
    if prefix_len is not None:
        if prefix is None:
            raise ValueError(op + ': prefix_len without a prefix')
        ctl.append(('prefix_len', prefix_len, torch.int32))
    if noise_row is not None:
        ctl.append(('noise_row', noise_row, torch.int32))
    if row_step0 is not None:
        # (uint32 counters travel as the int64 tensor the schema can carry)
        ctl.append(('row_step0', row_step0, torch.int64))
    _check_rows(op, n_seqs, dev, *ctl)
    if noise_row is not None and int(noise_row.min()) < 0:
        raise ValueError(op + ': noise_row must be >= 0')
    if row_step0 is not None:
        if int(row_step0.min()) < 0 or int(row_step0.max()) + T > 0xFFFFFFFF:
            raise ValueError(op + ': row_step0 + %d steps do not fit the 32-bit counter' % T)
        # the low words of the little-endian int64s: the library's uint32 array
        row_step0 = row_step0.view(torch.int32)[::2].contiguous()
    if step0 < 0 or step0 + T > 0xFFFFFFFF:
        raise ValueError(op + ': step0 %d + %d steps do not fit the 32-bit counter'
                         % (step0, T))
    n_forced = None
    if prefix is not None:
        if (prefix.dim() != 2 or prefix.shape[0] != n_seqs or prefix.shape[1] > T or
                prefix.dtype != torch.int64 or prefix.device != dev):
            raise ValueError(op + ': prefix must be an (n_seqs, <= %d) int64 tensor '
                             'on %s' % (T, dev))
        P = prefix.shape[1]
        n_forced = (prefix_len.clamp(0, P) if prefix_len is not None else
                    torch.full((n_seqs,), P, dtype=torch.int32, device=dev)).contiguous()
    if state is not None:
        if (state.dtype != torch.uint8 or state.dim() != 2 or state.shape[0] != n_seqs or
                state.device != dev):
            raise ValueError(op + ': state must be an (n_seqs, row_bytes) uint8 tensor '
                             'on %s' % dev)
        state = state.contiguous()
    return _generate(weights, meta, cond, row_bias, noise, seed, row_offset, flags, return_logp,
                     temperature, top_k, top_p, state, step0, prefix, n_forced, return_state,
                     noise_row, row_step0, return_scores)


@generate_stream.register_fake
def _(weights, meta, cond, row_bias, noise, seed, row_offset, flags, return_logp, temperature,
      top_k, top_p, state, step0, prefix, prefix_len, return_state):
    seq, logp = _generate_fake(meta, cond, return_logp)
    rows = (cond.shape[0], gen_state_row_bytes(meta)) if return_state else (0,)
    return seq, logp, cond.new_empty(rows, dtype=torch.uint8)


@torch.library.custom_op('srnn::generate_rows', mutates_args=())
def generate_rows(weights: list[Tensor], meta: list[int], cond: Tensor, row_bias: Tensor,
                  noise: Optional[Tensor], seed: int, row_offset: int, flags: int,
                  return_logp: bool, temperature: Optional[Tensor], top_k: Optional[Tensor],
                  top_p: Optional[Tensor], state: Optional[Tensor], step0: int,
                  prefix: Optional[Tensor], prefix_len: Optional[Tensor], return_state: bool,
                  noise_row: Optional[Tensor],
                  row_step0: Optional[Tensor]) -> tuple[Tensor, Tensor, Tensor]:
    """srnn::generate_stream whose rows have their own Philox origins (srnn_generate6):
      noise_row   (n_seqs,) int32 >= 0: the Philox row of local row b in place of
                  row_offset + b (equal values draw equal noise), or None
      row_step0   (n_seqs,) int64 in [0, 2^32 - T]: the Philox step of row b's first sample in
                  place of step0, or None
    Both only move Philox counters (a replayed `noise` and the log-probs keep their index from
    the call's first step); both None: srnn::generate_stream's call."""
    return _generate_stream('generate_rows', weights, meta, cond, row_bias, noise, seed,
                            row_offset, flags, return_logp, temperature, top_k, top_p, state, step0,
                            prefix, prefix_len, return_state, noise_row, row_step0)


@generate_rows.register_fake
def _(weights, meta, cond, row_bias, noise, seed, row_offset, flags, return_logp, temperature,
      top_k, top_p, state, step0, prefix, prefix_len, return_state, noise_row, row_step0):
    seq, logp = _generate_fake(meta, cond, return_logp)
    rows = (cond.shape[0], gen_state_row_bytes(meta)) if return_state else (0,)
    return seq, logp, cond.new_empty(rows, dtype=torch.uint8)


@torch.library.custom_op('srnn::generate_scored', mutates_args=())
def generate_scored(weights: list[Tensor], meta: list[int], cond: Tensor, row_bias: Tensor,
                    noise: Optional[Tensor], seed: int, row_offset: int, flags: int,
                    return_logp: bool, temperature: Optional[Tensor], top_k: Optional[Tensor],
                    top_p: Optional[Tensor], state: Optional[Tensor], step0: int,
                    prefix: Optional[Tensor], prefix_len: Optional[Tensor], return_state: bool,
                    noise_row: Optional[Tensor],
                    row_step0: Optional[Tensor]) -> tuple[Tensor, Tensor, Tensor, Tensor]:
    """srnn::generate_rows that also returns every step's score pair (srnn_generate7): the
    fourth result is (T, n_seqs, 2) float32, [..., 0] the log-prob of the step's sample (the
    forced one at a forced step; the dense logp gathered there, bit for bit) and [..., 1] the
    entropy of the model's softmax in nats, both whatever the controls did to the draw.  Runs
    the samplers' scored builds (level 3); the index stream is srnn::generate_rows'."""
    return _generate_stream('generate_scored', weights, meta, cond, row_bias, noise, seed,
                            row_offset, flags, return_logp, temperature, top_k, top_p, state, step0,
                            prefix, prefix_len, return_state, noise_row, row_step0, True)


@generate_scored.register_fake
def _(weights, meta, cond, row_bias, noise, seed, row_offset, flags, return_logp, temperature,
      top_k, top_p, state, step0, prefix, prefix_len, return_state, noise_row, row_step0):
    seq, logp = _generate_fake(meta, cond, return_logp)
    rows = (cond.shape[0], gen_state_row_bytes(meta)) if return_state else (0,)
    return (seq, logp, cond.new_empty(rows, dtype=torch.uint8),
            cond.new_empty((cond.shape[1] * meta[-1], cond.shape[0], 2)))


@torch.library.custom_op('srnn::gen_state_fresh', mutates_args=())
def gen_state_fresh(weights: list[Tensor], meta: list[int], n_seqs: int) -> Tensor:
    """(n_seqs, row_bytes) uint8 records of rows that have done no step (srnn_gen_state_fresh):
    a call of n_seqs rows from them is the call from no state, bit for bit."""
    import ctypes
    import model
    if n_seqs < 1:
        raise ValueError('gen_state_fresh: n_seqs must be >= 1')
    m = model.srnn_model_struct(weights, meta)
    dev = weights[0].device
    out = torch.empty((n_seqs, gen_state_row_bytes(meta)), dtype=torch.uint8, device=dev)
    sz = ctypes.c_size_t(0)
    H.lib().call('srnn_gen_workspace_size', ctypes.byref(m), n_seqs, ctypes.byref(sz))
    ws = torch.empty(sz.value, device=dev, dtype=torch.uint8)
    H.lib().call('srnn_gen_state_fresh', ctypes.byref(m), n_seqs, H.ptr(out), out.numel(),
                 H.ptr(ws), sz.value, H.stream())
    return out


@gen_state_fresh.register_fake
def _(weights, meta, n_seqs):
    return weights[0].new_empty((n_seqs, gen_state_row_bytes(meta)), dtype=torch.uint8)


# ------------------------------------------------------------------ generation sessions
def gen_session_open(weights, meta, n_seqs, max_frames, level, seed, row_offset, flags):
    """Opens a library session (srnn_gen_session_open) over model.generation_weights' tensors:
    returns (handle, arena).  The handle is a plain int; the caller keeps `arena` AND `weights`
    alive, and unchanged, until gen_session_close(handle) -- the session reads both."""
    import ctypes
    import model
    if n_seqs < 1 or max_frames < 1 or level not in (0, 1, 2, 3):
        raise ValueError('gen_session_open: n_seqs and max_frames must be >= 1, level 0, 1, 2 '
                         'or 3')
    if (level == 3) != bool(flags & H.GEN_SESSION_SCORE):
        raise ValueError('gen_session_open: level 3 and GEN_SESSION_SCORE go together')
    m = model.srnn_model_struct(weights, meta)
    dev = weights[0].device
    sz = ctypes.c_size_t(0)
    H.lib().call('srnn_gen_session_bytes', ctypes.byref(m), n_seqs, max_frames, level, flags,
                 ctypes.byref(sz))
    arena = torch.empty(sz.value, device=dev, dtype=torch.uint8)
    handle = ctypes.c_void_p(None)
    H.lib().call('srnn_gen_session_open', ctypes.byref(m), n_seqs, max_frames, level,
                 int(seed) & ((1 << 64) - 1), int(row_offset), flags, H.ptr(arena), sz.value,
                 H.stream(), ctypes.byref(handle))
    return handle.value, arena


def gen_session_close(handle):
    """Drains and releases a session (srnn_gen_session_close); its arena may then be freed."""
    H.lib().call('srnn_gen_session_close', handle)


def gen_session_stats(handle):
    """The session's diagnostic counters (srnn_gen_session_stats) as a dict."""
    import ctypes
    st = H.SrnnGenSessionStats()
    H.lib().call('srnn_gen_session_stats', handle, ctypes.byref(st))
    return {n: int(getattr(st, n)) for n, _ in st._fields_}


@torch.library.custom_op('srnn::gen_session_chunk', mutates_args=())
def gen_session_chunk(handle: int, lookback: int, cond: Tensor, row_bias: Optional[Tensor],
                      temperature: Optional[Tensor], top_k: Optional[Tensor],
                      top_p: Optional[Tensor], prefix: Optional[Tensor],
                      prefix_len: Optional[Tensor], noise_row: Optional[Tensor],
                      noise: Optional[Tensor], return_logp: bool) -> tuple[Tensor, Tensor]:
    """One chunk of a session (srnn_gen_session_chunk, then srnn_gen_session_sync): cond
    (n_seqs, frames, C) float32; every other tensor optional, None = as in the previous chunk
    (prefix: nothing forced): row_bias (n_seqs, D) float32, temperature / top_k / top_p as
    srnn::generate_ctrl_p takes them, prefix (n_seqs, P <= T) int64 with prefix_len (n_seqs,)
    int32 (None = P), noise_row a HOST (n_seqs,) int32 tensor of Philox rows, noise
    (T, n_seqs, 256) float32 for a session opened for replayed noise.  Returns (the chunk's
    sample indices (n_seqs, T) int64, log-probs (T, n_seqs, 256) or empty), T = frames *
    lookback.  The library checks the chunk against the session before it queues anything."""
    return _gen_session_chunk('gen_session_chunk', handle, lookback, cond, row_bias, temperature,
                              top_k, top_p, prefix, prefix_len, noise_row, noise, return_logp,
                              False)


def _gen_session_chunk(op, handle, lookback, cond, row_bias, temperature, top_k, top_p, prefix,
                       prefix_len, noise_row, noise, return_logp, return_scores):
    """The argument checks and the call of srnn::gen_session_chunk and its scored twin."""
    import ctypes
    if (cond.dim() != 3 or cond.dtype != torch.float32 or not cond.is_cuda or
            not cond.is_contiguous()):
        raise ValueError(op + ': cond must be a contiguous (n_seqs, frames, C) float32 device '
                         'tensor')
    n_seqs, frames, dev = cond.shape[0], cond.shape[1], cond.device
    T = frames * lookback
    _check_rows(op, n_seqs, dev,
                *[(n, t, dt) for n, t, dt in (('temperature', temperature, torch.float32),
                                              ('top_k', top_k, torch.int32),
                                              ('top_p', top_p, torch.float32),
                                              ('prefix_len', prefix_len, torch.int32))
                  if t is not None])
    if noise_row is not None:
        _check_rows(op, n_seqs, torch.device('cpu'), ('noise_row', noise_row, torch.int32))
    if row_bias is not None and (row_bias.dim() != 2 or row_bias.shape[0] != n_seqs or
                                 row_bias.dtype != torch.float32 or row_bias.device != dev or
                                 not row_bias.is_contiguous()):
        raise ValueError(op + ': row_bias must be a contiguous (n_seqs, D) float32 tensor on %s'
                         % dev)
    if noise is not None and (noise.shape != (T, n_seqs, 256) or noise.dtype != torch.float32 or
                              noise.device != dev or not noise.is_contiguous()):
        raise ValueError(op + ': noise must be a contiguous (%d, %d, 256) float32 tensor on %s'
                         % (T, n_seqs, dev))
    ck = H.SrnnGenChunk()
    if prefix_len is not None and prefix is None:
        raise ValueError(op + ': prefix_len without a prefix')
    if prefix is not None:
        if (prefix.dim() != 2 or prefix.shape[0] != n_seqs or not 1 <= prefix.shape[1] <= T or
                prefix.dtype != torch.int64 or prefix.device != dev):
            raise ValueError(op + ': prefix must be an (n_seqs, 1..%d) int64 tensor on %s'
                             % (T, dev))
        P = prefix.shape[1]
        prefix = prefix.clamp(0, 255).contiguous()
        n_forced = (prefix_len.clamp(0, P) if prefix_len is not None else
                    torch.full((n_seqs,), P, dtype=torch.int32, device=dev)).contiguous()
        ck.prefix, ck.prefix_cols, ck.n_forced = H.ptr(prefix), P, H.ptr(n_forced)
    seq = torch.empty((n_seqs, T), dtype=torch.long, device=dev)
    logp = torch.empty((T, n_seqs, 256) if return_logp else (0,), device=dev)
    ck.n_frames, ck.cond, ck.row_bias = frames, H.ptr(cond), H.ptr(row_bias)
    ck.temperature, ck.top_k, ck.top_p = H.ptr(temperature), H.ptr(top_k), H.ptr(top_p)
    ck.noise_row, ck.noise = H.ptr(noise_row), H.ptr(noise)
    ck.seq_out, ck.logp_out = H.ptr(seq), H.ptr(logp) if return_logp else None
    if return_scores:
        score = torch.empty((T, n_seqs, 2), device=dev)
        H.lib().call('srnn_gen_session_chunk2', handle, ctypes.byref(ck), H.ptr(score),
                     H.stream())
        H.lib().call('srnn_gen_session_sync', handle)
        return seq, logp, score
    H.lib().call('srnn_gen_session_chunk', handle, ctypes.byref(ck), H.stream())
    H.lib().call('srnn_gen_session_sync', handle)
    return seq, logp


@gen_session_chunk.register_fake
def _(handle, lookback, cond, row_bias, temperature, top_k, top_p, prefix, prefix_len, noise_row,
      noise, return_logp):
    n_seqs, T = cond.shape[0], cond.shape[1] * lookback
    return (cond.new_empty((n_seqs, T), dtype=torch.long),
            cond.new_empty((T, n_seqs, 256) if return_logp else (0,)))


@torch.library.custom_op('srnn::gen_session_chunk_scored', mutates_args=())
def gen_session_chunk_scored(handle: int, lookback: int, cond: Tensor,
                             row_bias: Optional[Tensor], temperature: Optional[Tensor],
                             top_k: Optional[Tensor], top_p: Optional[Tensor],
                             prefix: Optional[Tensor], prefix_len: Optional[Tensor],
                             noise_row: Optional[Tensor], noise: Optional[Tensor],
                             return_logp: bool) -> tuple[Tensor, Tensor, Tensor]:
    """srnn::gen_session_chunk of a session opened for scores (srnn_gen_session_chunk2): also
    returns the chunk's (T, n_seqs, 2) score pairs, srnn::generate_scored's.  The library
    refuses it, with nothing queued, on a session opened without GEN_SESSION_SCORE."""
    return _gen_session_chunk('gen_session_chunk_scored', handle, lookback, cond, row_bias,
                              temperature, top_k, top_p, prefix, prefix_len, noise_row, noise,
                              return_logp, True)


@gen_session_chunk_scored.register_fake
def _(handle, lookback, cond, row_bias, temperature, top_k, top_p, prefix, prefix_len, noise_row,
      noise, return_logp):
    n_seqs, T = cond.shape[0], cond.shape[1] * lookback
    return (cond.new_empty((n_seqs, T), dtype=torch.long),
            cond.new_empty((T, n_seqs, 256) if return_logp else (0,)),
            cond.new_empty((T, n_seqs, 2)))


@torch.library.custom_op('srnn::gen_session_state', mutates_args=())
def gen_session_state(handle: int, like: Tensor, n_seqs: int, row_bytes: int) -> Tensor:
    """The session's records (srnn_gen_session_state_get) as an (n_seqs, row_bytes) uint8 tensor
    on `like`'s device, after the chunks queued so far."""
    out = torch.empty((n_seqs, row_bytes), dtype=torch.uint8, device=like.device)
    H.lib().call('srnn_gen_session_state_get', handle, H.ptr(out), out.numel())
    return out


@gen_session_state.register_fake
def _(handle, like, n_seqs, row_bytes):
    return like.new_empty((n_seqs, row_bytes), dtype=torch.uint8)


def gen_session_replace(handle, rows, records):
    """Replaces the records of the session's rows `rows` (a host (n,) int32 tensor of distinct
    row numbers) by `records` ((n, row_bytes) uint8 on the device): srnn_gen_session_state_set_rows,
    which checks every header before it writes anything."""
    if (rows.dtype != torch.int32 or rows.dim() != 1 or rows.is_cuda or not rows.is_contiguous()):
        raise ValueError('gen_session_replace: rows must be a contiguous host (n,) int32 tensor')
    if (records.dtype != torch.uint8 or records.dim() != 2 or not records.is_cuda or
            records.shape[0] != rows.shape[0]):
        raise ValueError('gen_session_replace: records must be an (n, row_bytes) uint8 device '
                         'tensor, one record per row number')
    records = records.contiguous()
    H.lib().call('srnn_gen_session_state_set_rows', handle, H.ptr(rows), rows.shape[0],
                 H.ptr(records), records.numel(), H.stream())


@torch.library.custom_op('srnn::sample_rows', mutates_args=())
def sample_rows(logits: Tensor, noise: Optional[Tensor], seed: int, row0: int, step: int,
                temperature: Optional[Tensor], top_k: Optional[Tensor],
                top_p: Optional[Tensor], return_logp: bool) -> tuple[Tensor, Tensor]:
    """One draw per row of logits (rows, 256) float32 (row stride a multiple of 4 floats) by the
    generation loops' sampler (srnn_sample_rows): ((rows,) int64 indices, (rows, 256) float32
    log_softmax(logits) or empty).  noise (rows, 256) float32 Exp(1) or None = Philox with
    (seed, row0, step); temperature / top_k / top_p (rows,) float32 / int32 / float32 or None,
    at whose level the draw runs (all None: the plain draw)."""
    return _sample_rows(logits, noise, seed, row0, step, temperature, top_k, top_p, return_logp,
                        False)


def _sample_rows(logits, noise, seed, row0, step, temperature, top_k, top_p, return_logp,
                 return_scores):
    """The argument checks and the call of srnn::sample_rows and srnn::sample_rows_scored."""
    if (logits.dim() != 2 or logits.shape[1] != 256 or logits.dtype != torch.float32 or
            not logits.is_cuda or logits.stride(1) != 1 or logits.shape[0] < 1):
        raise ValueError('sample_rows: logits must be a (rows, 256) float32 device tensor with '
                         'unit column stride')
    rows, dev = logits.shape[0], logits.device
    if rows > 1 and (logits.stride(0) < 256 or logits.stride(0) % 4):
        raise ValueError('sample_rows: logits row stride must be >= 256 and a multiple of 4')
    if noise is not None and (noise.shape != (rows, 256) or noise.dtype != torch.float32 or
                              noise.device != dev or not noise.is_contiguous()):
        raise ValueError('sample_rows: noise must be a contiguous (%d, 256) float32 tensor on %s'
                         % (rows, dev))
    if row0 < 0 or step < 0:
        raise ValueError('sample_rows: row0 and step must be >= 0')
    _check_rows('sample_rows', rows, dev,
                *[(n, t, dt) for n, t, dt in (('temperature', temperature, torch.float32),
                                              ('top_k', top_k, torch.int32),
                                              ('top_p', top_p, torch.float32)) if t is not None])
    idx = torch.empty(rows, device=dev, dtype=torch.int64)
    logp = torch.empty((rows, 256) if return_logp else (0,), device=dev, dtype=torch.float32)
    args = (H.ptr(logits), logits.stride(0) if rows > 1 else 256, rows,
            H.ptr(noise), int(seed) & ((1 << 64) - 1), int(row0), int(step),
            H.ptr(temperature), H.ptr(top_k), H.ptr(top_p), H.ptr(idx),
            H.ptr(logp) if return_logp else None, H.stream())
    if return_scores:
        score = torch.empty((rows, 2), device=dev, dtype=torch.float32)
        H.lib().call('srnn_sample_rows2', *args, H.ptr(score))
        return idx, logp, score
    H.lib().call('srnn_sample_rows', *args)
    return idx, logp


@sample_rows.register_fake
def _(logits, noise, seed, row0, step, temperature, top_k, top_p, return_logp):
    rows = logits.shape[0]
    return (logits.new_empty((rows,), dtype=torch.int64),
            logits.new_empty((rows, 256) if return_logp else (0,)))


@torch.library.custom_op('srnn::sample_rows_scored', mutates_args=())
def sample_rows_scored(logits: Tensor, noise: Optional[Tensor], seed: int, row0: int, step: int,
                       temperature: Optional[Tensor], top_k: Optional[Tensor],
                       top_p: Optional[Tensor],
                       return_logp: bool) -> tuple[Tensor, Tensor, Tensor]:
    """srnn::sample_rows that also returns the rows' (rows, 2) float32 score pairs
    (srnn_sample_rows2): the log-prob of the index drawn (logp gathered there, bit for bit) and
    the entropy of softmax(logits) in nats, whatever the controls.  The draw is the scored
    build's (level 3), which draws srnn::sample_rows' index."""
    return _sample_rows(logits, noise, seed, row0, step, temperature, top_k, top_p, return_logp,
                        True)


@sample_rows_scored.register_fake
def _(logits, noise, seed, row0, step, temperature, top_k, top_p, return_logp):
    rows = logits.shape[0]
    return (logits.new_empty((rows,), dtype=torch.int64),
            logits.new_empty((rows, 256) if return_logp else (0,)),
            logits.new_empty((rows, 2)))


OPS = ('tier_fwd', 'tier_bwd', 'mlp_fwd', 'mlp_bwd', 'nll_bits', 'nll_bits_bwd', 'upsample',
       'upsample_bwd', 'dequant', 'adam_clip_', 'step_advance_', 'generate', 'generate_ctrl',
       'generate_ctrl_p', 'generate_stream', 'generate_rows', 'gen_state_fresh', 'sample_rows',
       'gen_session_chunk', 'gen_session_state', 'generate_scored', 'sample_rows_scored',
       'gen_session_chunk_scored')
