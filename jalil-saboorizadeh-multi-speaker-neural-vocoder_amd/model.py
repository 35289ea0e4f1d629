"""Drop-in for the reference's model.py (model.py:1-520), MI355X-native.

Same classes, constructor signatures, attributes, state_dict keys and init recipe
(RNG consumption order) as the reference -- SampleRNN, FrameLevelRNN, SampleLevelMLP,
Runner, Predictor, Generator -- so train.py / generate.py bind unchanged.  Every
forward/backward runs on the hand-written HIP kernels of libsamplernn_hip.so:

  * FrameLevelRNN  -> srnn::tier_fwd / tier_bwd (custom_ops.py; tier_forward /
    tier_backward here): input / cond / speaker projections (MFMA GEMMs with fused bias +
    upper-tier add), the GRU input projection for all frames in one GEMM, the recurrence as
    one persistent sweep per layer (gru_xcd.hip) or per-step kernels, LearnedUpsampling1d as
    one GEMM; the backward mirrors it.
  * SampleLevelMLP -> srnn::mlp_fwd / mlp_bwd (mlp_forward / mlp_backward): embedding . conv
    folded into a per-tap table, L1 as a gather-sum, hidden / output GEMMs with fused bias /
    ReLU, log-softmax kernel; with sequence_nll_loss_bits the loss backward is fused in.
  * Generator      -> srnn::generate: the whole autoregressive loop on the device (persistent
    sample loop + tier ticks, captured as a hipGraph; no per-sample host round trip).

Numerics: fp32 by default (parity mode, logits within 1e-4 of the reference);
`SampleRNN.compute_dtype = torch.bfloat16` (or env SRNN_COMPUTE_DTYPE=bf16) runs the
matmuls on bf16 MFMA with fp32 accumulation, fp32 master weights and fp32 recurrences.
"""
import ctypes
import math
import os

import numpy as np
import torch
from torch.nn import init

import custom_ops
import nn
import utils
import samplernn_hip as H

verbose = False
# (tests) how often a fused side result was consumed, and which recurrence kernels ran
_STATS = {'fused_colsum': 0, 'fused_lp': 0, 'csum_epi': 0, 'lsm_epi': 0, 'gru_xcd_fwd': 0, 'gru_xcd_bwd': 0, 'gru_seq': 0,
          'gru_cell_steps': 0, 'gru_cell_bwd_steps': 0, 'out_bwd_fused': 0}


def _default_dtype():
    v = os.environ.get('SRNN_COMPUTE_DTYPE', 'fp32').lower()
    return torch.bfloat16 if v in ('bf16', 'bfloat16') else torch.float32


class _GRUParams(torch.nn.Module):
    """Parameter container with torch.nn.GRU's names and reset_parameters RNG order
    (weight_ih_l{l}, weight_hh_l{l}, bias_ih_l{l}, bias_hh_l{l}); the recurrence itself
    runs in the HIP gru_cell kernel."""

    def __init__(self, input_size, hidden_size, num_layers):
        super().__init__()
        self.input_size, self.hidden_size, self.num_layers = input_size, hidden_size, num_layers
        for l in range(num_layers):
            isz = input_size if l == 0 else hidden_size
            self.register_parameter('weight_ih_l%d' % l,
                                    torch.nn.Parameter(torch.empty(3 * hidden_size, isz)))
            self.register_parameter('weight_hh_l%d' % l,
                                    torch.nn.Parameter(torch.empty(3 * hidden_size, hidden_size)))
            self.register_parameter('bias_ih_l%d' % l,
                                    torch.nn.Parameter(torch.empty(3 * hidden_size)))
            self.register_parameter('bias_hh_l%d' % l,
                                    torch.nn.Parameter(torch.empty(3 * hidden_size)))
        stdv = 1.0 / np.sqrt(hidden_size)
        for p in self.parameters():
            init.uniform_(p, -stdv, stdv)


class SampleRNN(torch.nn.Module):
    """model.py:18-62."""

    def __init__(self, frame_sizes, n_rnn, dim, learn_h0, q_levels, ulaw, weight_norm, cond_dim,
                 spk_dim, qrnn=False):
        super().__init__()
        self.dim = dim
        self.q_levels = q_levels
        self.ulaw = ulaw
        self.cond_dim = cond_dim
        self.spk_dim = spk_dim
        self.frame_sizes = [int(f) for f in frame_sizes]
        self.n_rnn = n_rnn
        self.compute_dtype = _default_dtype()
        self.dequantize = utils.udequantize if ulaw else utils.linear_dequantize
        ns_frame_samples = list(map(int, np.cumprod(frame_sizes)))
        is_cond = [False] * len(frame_sizes)
        is_cond[-1] = True
        self.frame_level_rnns = torch.nn.ModuleList([
            FrameLevelRNN(frame_size, n_frame_samples, n_rnn, dim, learn_h0, c, cond_dim,
                          spk_dim, weight_norm, qrnn)
            for (frame_size, n_frame_samples, c) in zip(frame_sizes, ns_frame_samples, is_cond)
        ])
        self.sample_level_mlp = SampleLevelMLP(frame_sizes[0], dim, q_levels, weight_norm)
        self.frame_level_rnns[0].__dict__['_feeds_mlp'] = True
        for m in self.modules():
            if m is not self:
                m.__dict__['_root'] = self

    @property
    def lookback(self):
        return self.frame_level_rnns[-1].n_frame_samples


class FrameLevelRNN(torch.nn.Module):
    """model.py:65-263 (parameters, init recipe, forward contract)."""

    def __init__(self, frame_size, n_frame_samples, n_rnn, dim, learn_h0, is_cond, cond_dim,
                 spk_dim, w_norm, qrnn):
        super().__init__()
        self.frame_size = frame_size
        self.n_frame_samples = n_frame_samples
        self.dim = dim
        self.cond_dim = cond_dim
        self.spk_dim = spk_dim
        self.weight_norm = w_norm
        self.qrnn = qrnn
        self.n_rnn = n_rnn
        self.is_cond = is_cond
        h0 = torch.zeros(n_rnn, dim)
        if learn_h0:
            self.h0 = torch.nn.Parameter(h0)
        else:
            self.register_buffer('h0', h0)
        self.input_expand = torch.nn.Conv1d(n_frame_samples, dim, kernel_size=1)
        if is_cond:
            self.cond_expand = torch.nn.Conv1d(cond_dim, dim, kernel_size=1)
            init.kaiming_uniform_(self.cond_expand.weight)
            init.constant_(self.cond_expand.bias, 0)
            self.spk_embedding = torch.nn.Embedding(spk_dim, spk_dim)
            self.spk_expand = torch.nn.Conv1d(spk_dim, dim, kernel_size=1)
            init.kaiming_uniform_(self.spk_expand.weight)
            init.constant_(self.spk_expand.bias, 0)
            if w_norm:
                nn.apply_weight_norm(self.cond_expand)
                nn.apply_weight_norm(self.spk_expand)
        else:
            self.cond_expand = None
            self.spk_expand = None
            self.spk_embedding = None
        init.kaiming_uniform_(self.input_expand.weight)
        init.constant_(self.input_expand.bias, 0)
        if w_norm:
            nn.apply_weight_norm(self.input_expand)
        # qrnn=True in the reference also builds a torch GRU (model.py:133-139)
        self.rnn = _GRUParams(dim, dim, n_rnn)
        for i in range(n_rnn):
            nn.concat_init(getattr(self.rnn, 'weight_ih_l%d' % i),
                           [nn.lecun_uniform, nn.lecun_uniform, nn.lecun_uniform])
            init.constant_(getattr(self.rnn, 'bias_ih_l%d' % i), 0)
            nn.concat_init(getattr(self.rnn, 'weight_hh_l%d' % i),
                           [nn.lecun_uniform, nn.lecun_uniform, init.orthogonal_])
            init.constant_(getattr(self.rnn, 'bias_hh_l%d' % i), 0)
        self.upsampling = nn.LearnedUpsampling1d(dim, dim, frame_size)
        init.uniform_(self.upsampling.conv_t.weight, -np.sqrt(6 / dim), np.sqrt(6 / dim))
        init.constant_(self.upsampling.bias, 0)
        # always weight-normed: model.py:177 tests the imported function, not the flag
        nn.apply_weight_norm(self.upsampling.conv_t)

    # parameter tensors in the order tier_forward consumes them (srnn::tier_fwd's params)
    def _param_list(self):
        ps = []
        ps += nn.weight_params(self.input_expand) + [self.input_expand.bias]
        if self.is_cond:
            ps += nn.weight_params(self.cond_expand) + [self.cond_expand.bias]
            ps += [self.spk_embedding.weight]
            ps += nn.weight_params(self.spk_expand) + [self.spk_expand.bias]
        for l in range(self.n_rnn):
            ps += [getattr(self.rnn, 'weight_ih_l%d' % l), getattr(self.rnn, 'weight_hh_l%d' % l),
                   getattr(self.rnn, 'bias_ih_l%d' % l), getattr(self.rnn, 'bias_hh_l%d' % l)]
        ps += nn.weight_params(self.upsampling.conv_t) + [self.upsampling.bias]
        return ps

    def forward(self, prev_samples, upper_tier_conditioning, hidden, cond, spk, writer,
                iterations):
        """model.py:180-263: (B,F,nfs) samples -> ((B, F*frame_size, D) conditioning, hidden)."""
        H.need_cuda(prev_samples)
        dev = prev_samples.device
        if cond is not None:
            cond = cond.to(dev)
        if spk is not None:
            spk = spk.to(dev).long()
        h0 = self.h0
        ps = self._param_list()
        # the registered op srnn::tier_fwd (custom_ops.py; autograd: srnn::tier_bwd)
        out, h = custom_ops.tier(prev_samples.float().contiguous(),
                                 None if upper_tier_conditioning is None
                                 else upper_tier_conditioning.contiguous(),
                                 cond, spk, None if hidden is None else hidden.contiguous(),
                                 h0, ps, tier_meta(self))
        return out, h


def _wcast(mod, T):
    """Effective weight of a conv module in the compute dtype: the cached copy of the plain
    parameter (samplernn_hip.cast_param), or a cast of the weight-normed weight."""
    if hasattr(mod, 'weight_g'):
        return H.cast(nn.weight_of(mod), T)
    return H.cast_param(mod.weight, T)


def _wcast_t(mod, T):
    """Transposed effective weight (in, out) of a k = 1 conv in the compute dtype, permuted
    straight from the fp32 weight (one launch; weight norm applied first)."""
    w = nn.weight_of(mod)
    o, i = w.shape[0], w.shape[1]
    return H.permute3(w.reshape(1, o, i), (0, 2, 1), dtype=T).reshape(i, o)


def _dt(mod):
    T = mod.__dict__.get('T')
    if T is not None:
        return T
    root = mod.__dict__.get('_root')
    return root.compute_dtype if root is not None else torch.float32


class _Conv:
    """A conv's parameters as the weight helpers of nn.py see them: `weight`, or
    `weight_g` / `weight_v` under weight norm."""

    def __init__(self, ts):
        if len(ts) == 2:
            self.weight_g, self.weight_v = ts
        else:
            self.weight = ts[0]


class TierSpec:
    """Static description of one FrameLevelRNN for the srnn::tier_* ops: the meta ints
    (tier_meta) plus the parameter list in FrameLevelRNN._param_list order."""

    def __init__(self, meta, ps):
        (self.dim, self.n_frame_samples, self.frame_size, self.n_rnn, is_cond, feeds, dt,
         wn_ie, wn_c, wn_s, wn_up) = [int(v) for v in meta[:11]]
        self.is_cond = bool(is_cond)
        self.T = torch.bfloat16 if dt else torch.float32
        self._feeds_mlp = bool(feeds)
        it = iter(ps)

        def take(wn):
            return _Conv([next(it) for _ in range(2 if wn else 1)])
        self.input_expand = take(wn_ie)
        next(it)
        if self.is_cond:
            self.cond_expand = take(wn_c)
            next(it)
            next(it)
            self.spk_expand = take(wn_s)
            next(it)
        for _ in range(4 * self.n_rnn):
            next(it)
        self.upsampling = _State()
        self.upsampling.conv_t = take(wn_up)


def tier_meta(mod):
    """The meta ints of TierSpec for a FrameLevelRNN."""
    wn = lambda m: int(hasattr(m, 'weight_g'))  # noqa: E731
    return [mod.dim, mod.n_frame_samples, mod.frame_size, mod.n_rnn, int(mod.is_cond),
            int(bool(mod.__dict__.get('_feeds_mlp'))), H.dcode(_dt(mod)),
            wn(mod.input_expand), wn(mod.cond_expand) if mod.is_cond else 0,
            wn(mod.spk_expand) if mod.is_cond else 0, wn(mod.upsampling.conv_t)]


class MlpSpec:
    """Static description of the SampleLevelMLP for the srnn::mlp_* ops (mlp_meta + the
    parameter list in SampleLevelMLP._param_list order)."""

    def __init__(self, meta, ps):
        self.q_levels, self.dim, self.frame_size, dt, wn = [int(v) for v in meta[:5]]
        self.T = torch.bfloat16 if dt else torch.float32
        it = iter(ps)

        def take():
            return _Conv([next(it) for _ in range(2 if wn else 1)])
        self.embedding = _Conv([next(it)])
        self.input = take()
        self.hidden = take()
        self.hidden.bias = next(it)
        self.output = take()
        self.output.bias = next(it)


def mlp_meta(mlp):
    return [mlp.q_levels, mlp.dim, mlp.frame_size, H.dcode(_dt(mlp)),
            int(hasattr(mlp.hidden, 'weight_g'))]


class _State:
    """What a tier / MLP forward keeps for its backward (custom_ops stash)."""


def _gru_layer_forward(T, B, D, Fr, gi, h0, whh, b_hh):
    """One GRU layer over all Fr steps (srnn_gru_layer_fwd: the library plans the back end --
    a persistent sweep or one cell launch per step).  gi (B*Fr, 3D) fp32, h0 (B, D) fp32.
    Returns out (fp32), its T copy (out itself in fp32), the saved gates, and -- from the XCD
    sweep only, else None -- the previous-state sequence [h0, h_0 .. h_{F-2}] in T that the
    backward's W_hh gradient consumes."""
    dev = gi.device
    lp = T != torch.float32
    be, nwork, _ = H.gru_layer_plan(T, B, D)
    out = torch.empty((B, Fr, D), device=dev, dtype=torch.float32)
    outT = torch.empty((B, Fr, D), device=dev, dtype=T) if lp else out
    gt = torch.empty((B, Fr, 4 * D), device=dev, dtype=torch.float32)
    hprevT = torch.empty((B, Fr, D), device=dev, dtype=T) if be == 'xcd' else None
    work = torch.empty(nwork, device=dev, dtype=torch.uint8) if nwork else None
    if be != 'steps':
        H.before_persistent_sweep()
    _STATS[{'xcd': 'gru_xcd_fwd', 'seq': 'gru_seq', 'steps': 'gru_cell_steps'}[be]] += \
        Fr if be == 'steps' else 1
    ev = H.roof_begin() if be == 'xcd' else None
    H.lib().call('srnn_gru_layer_fwd', H.dcode(T), B, D, Fr, H.ptr(gi), Fr * 3 * D, 3 * D,
                 H.ptr(h0), H.ptr(whh), H.ptr(b_hh), H.ptr(out), H.ptr(outT) if lp else None,
                 Fr * D, D, H.ptr(gt), Fr * 4 * D, 4 * D, H.ptr(hprevT), H.ptr(work), nwork,
                 H.stream())
    H.roof_end('gru_xcd_fwd', ev, 2.0 * B * Fr * 3 * D * D)
    return out, outT, gt, hprevT


def _gru_layer_backward(T, B, D, Fr, dOut, gates, out, h0, whh, whhT):
    """Reverse sweep of one GRU layer (srnn_gru_layer_bwd, the same plan as the forward).
    Returns (dGH, dGHT, dGI, dGIT, bsum, ddir0) in one of two forms.  Under the XCD plan the
    sweep writes the GEMM operands dGHT / dGIT (T) and per-row bias sums bsum (B, 4D), no
    fp32 copies of either (dGH, dGI None); under the others fp32 dGH / dGI and dGHT (the T
    copy of dGH; dGH itself in fp32), with dGIT and bsum None.  ddir0: dh_direct of step 0."""
    dev = dOut.device
    lp = T != torch.float32
    be, _, nwork = H.gru_layer_plan(T, B, D)
    g3 = (B, Fr, 3 * D)
    dGH = dGI = dGIT = bsum = None
    if be == 'xcd':
        dGHT = torch.empty(g3, device=dev, dtype=T)
        dGIT = torch.empty(g3, device=dev, dtype=T)
        bsum = torch.empty((B, 4 * D), device=dev, dtype=torch.float32)
    else:
        dGH = torch.empty(g3, device=dev, dtype=torch.float32)
        dGHT = torch.empty(g3, device=dev, dtype=T) if lp else dGH
        dGI = torch.empty(g3, device=dev, dtype=torch.float32)
    ddir0 = torch.empty((B, D), device=dev, dtype=torch.float32)
    work = torch.empty(nwork, device=dev, dtype=torch.uint8) if nwork else None
    dOut = dOut.contiguous()
    if be != 'steps':
        H.before_persistent_sweep()       # (DP: in-flight all-reduces finish first)
    else:
        _STATS['gru_cell_bwd_steps'] += Fr
    ev = None
    if be == 'xcd':
        _STATS['gru_xcd_bwd'] += 1
        ev = H.roof_begin()
    H.lib().call('srnn_gru_layer_bwd', H.dcode(T), B, D, Fr, H.ptr(dOut), Fr * D, D,
                 H.ptr(gates), Fr * 4 * D, 4 * D, H.ptr(out), Fr * D, D, H.ptr(h0), H.ptr(whh),
                 H.ptr(whhT), H.ptr(dGH), H.ptr(dGHT) if lp else None, H.ptr(dGI), H.ptr(dGIT),
                 H.ptr(bsum), Fr * 3 * D, 3 * D, H.ptr(ddir0), H.ptr(work), nwork, H.stream())
    # (the dgh_{t+1} W_hh products of steps 1 .. F-1; step F-1 has none)
    H.roof_end('gru_xcd_bwd', ev, 2.0 * B * (Fr - 1) * 3 * D * D)
    if be != 'steps':
        H.after_persistent_sweep()        # (DP: gradient buckets ready before it go out now)
    return dGH, dGHT, dGI, dGIT, bsum, ddir0


def tier_forward(mod, prev, upper, cond, spk, hidden, h0, ps):
    """FrameLevelRNN forward (model.py:180-263) on the HIP kernels: returns (Y, h_new, state)
    with state what tier_backward needs (srnn::tier_fwd, custom_ops.py)."""
    T = _dt(mod)
    B, Fr, nfs = prev.shape
    D = mod.dim
    L = mod.n_rnn
    dev = prev.device
    it = iter(ps)

    def take_w(m):
        return [next(it) for _ in nn.weight_params(m)]

    ie_p = take_w(mod.input_expand)
    ie_b = next(it)
    W_ie = _wcast(mod.input_expand, T).reshape(D, nfs)
    prevT = H.cast(prev.reshape(B * Fr, nfs), T)
    lp = T != torch.float32
    # In the low-precision mode only the compute-dtype copy of the first GRU layer's input
    # is ever read, so the last projection writes it directly (no fp32 x0, no cast); the
    # fp32 (parity) mode keeps the reference's summation order.
    x0 = H.linear(prevT, W_ie, bias=ie_b,
                  cin=None if upper is None else upper.reshape(B * Fr, D),
                  beta=0.0 if upper is None else 1.0,
                  out_dtype=T if lp and not mod.is_cond else torch.float32)
    condT = spk_embT = W_c = W_s = None
    if mod.is_cond:
        take_w(mod.cond_expand)
        c_b = next(it)
        E_s = next(it)
        take_w(mod.spk_expand)
        s_b = next(it)
        C = cond.shape[-1]
        W_c = _wcast(mod.cond_expand, T).reshape(D, C)
        condT = H.cast(cond.reshape(B * Fr, C).float().contiguous(), T)
        S = E_s.shape[1]
        spk_flat = spk.reshape(B).contiguous()
        spk_emb = torch.empty((B, S), device=dev, dtype=torch.float32)
        H.lib().call('srnn_gather_rows', H.ptr(E_s), S, H.ptr(spk_flat), B, S, H.ptr(spk_emb),
                     H.F32, S, H.stream())
        spk_embT = H.cast(spk_emb, T)
        W_s = _wcast(mod.spk_expand, T).reshape(D, S)
        spk_proj = H.linear(spk_embT, W_s, bias=s_b)
        if lp:
            H.lib().call('srnn_add_bcast_rows', H.ptr(x0), H.ptr(spk_proj), B, Fr, D, D,
                         H.stream())
            x0 = H.linear(condT, W_c, bias=c_b, cin=x0, beta=1.0, out_dtype=T)
        else:
            H.linear(condT, W_c, bias=c_b, cin=x0, beta=1.0, out=x0)
            H.lib().call('srnn_add_bcast_rows', H.ptr(x0), H.ptr(spk_proj), B, Fr, D, D,
                         H.stream())
    else:
        spk_flat = None
    reset = hidden is None
    if reset:   # model.py:224-228
        h_in = h0.detach().reshape(L, 1, D).expand(L, B, D).contiguous()
    else:
        h_in = hidden.float().contiguous()
    Wih, Whh, WhhF, bih, bhh = [], [], [], [], []
    xs, outs, outsT, gates, hprevs = [], [], [], [], []
    X = x0
    for l in range(L):
        wih, whh, b_ih, b_hh = next(it), next(it), next(it), next(it)
        Wih.append(H.cast_param(wih, T))
        Whh.append(H.cast_param(whh, T))
        WhhF.append(whh)
        bih.append(b_ih)
        bhh.append(b_hh)
        XT = H.cast(X, T)
        gi = H.linear(XT, Wih[l], bias=b_ih)                      # (B*F, 3D)
        out, outT, gt, hprevT = _gru_layer_forward(T, B, D, Fr, gi, h_in[l], Whh[l], b_hh)
        xs.append(XT)
        hprevs.append(hprevT)
        outs.append(out)
        outsT.append(outT)
        gates.append(gt)
        X = out.reshape(B * Fr, D)
    up_p = take_w(mod.upsampling.conv_t)
    up_b = next(it)
    k = mod.frame_size
    W_up = nn.convt_operand(mod.upsampling.conv_t, T)                        # (k, D, D)
    b_up = H.permute3(up_b.reshape(1, D, k), (0, 2, 1)).reshape(k * D)
    # the bottom tier feeds the MLP's gather directly: its upsampled output (and so the
    # gradient coming back) is in the compute dtype; upper tiers stay fp32 (Cin input)
    y_dt = T if mod.__dict__.get('_feeds_mlp') else torch.float32
    Y = H.linear(outsT[-1].reshape(B * Fr, D), W_up.reshape(k * D, D), bias=b_up,
                 out_dtype=y_dt)
    h_new = torch.stack([o[:, -1] for o in outs], 0)
    ctx = _State()
    ctx.mod = mod
    ctx.reset = reset
    ctx.has_upper = upper is not None
    ctx.dims = (B, Fr, nfs, D, L, k)
    ctx.T = T
    ctx.saved_tensors = (prevT, condT, spk_embT, spk_flat, h_in, W_ie, W_c, W_s, W_up,
                         *Wih, *Whh, *xs, *outs, *outsT, *gates, *WhhF, *hprevs)
    return Y.reshape(B, Fr * k, D), h_new, ctx


def tier_backward(ctx, dY, need_h0):
    """Backward of tier_forward: (d_upper or None, dh0 or None, [parameter gradients in
    _param_list order])."""
    mod = ctx.mod
    B, Fr, nfs, D, L, k = ctx.dims
    T = ctx.T
    lp = T != torch.float32
    sv = ctx.saved_tensors
    prevT, condT, spk_embT, spk_flat, h_in, W_ie, W_c, W_s, W_up = sv[:9]
    r = sv[9:]
    Wih, Whh = r[:L], r[L:2 * L]
    xs, outs, outsT, gates = r[2 * L:3 * L], r[3 * L:4 * L], r[4 * L:5 * L], r[5 * L:6 * L]
    WhhF = r[6 * L:7 * L]                     # the fp32 parameters W_hh
    hprevs = r[7 * L:8 * L]                   # [h_in, out[:, :F-1]] in T, or None
    dev = dY.device
    st = H.stream
    M = B * Fr
    # --- upsampling (nn.py:33-43)
    if dY.dtype == T:
        dY2 = dYT = dY.reshape(M, k * D).contiguous()
    else:
        dY2 = dY.reshape(M, k * D).float().contiguous()
        # the tier below already cast this gradient (its dx0) to the compute dtype
        lpc = getattr(dY, '_srnn_lp', None)
        if lpc is not None and lpc[1] == dY._version and lpc[0].dtype == T and \
                lpc[0].numel() == dY2.numel() and dY2.data_ptr() == dY.data_ptr():
            dYT = lpc[0].reshape(M, k * D)
            _STATS['fused_lp'] += 1
        else:
            dYT = H.cast(dY2, T)
    # weight gradient transposed, [i][j*D + o]: one row per input channel for the
    # per-channel weight-norm backward (no permute of the 16 x D x D gradient)
    dWupT = H.gemm(outsT[-1].reshape(M, D), dYT, transA=True)         # (D, k*D)
    # bias gradient: summed by the MLP's dTab pass when dY is its untouched d(upper)
    cs = getattr(dY, '_srnn_colsum', None)
    if cs is not None and cs[1] == dY._version and cs[2] == k and cs[0].numel() == k * D:
        db_up = cs[0]
        _STATS['fused_colsum'] += 1
    else:
        db_up = H.colsum(dY2, M, k * D)
    dX = H.gemm(dYT, W_up.reshape(k * D, D))                          # (M, D)
    g_up = nn.convt_grad_to_params(mod.upsampling.conv_t, dWupT)
    g_up_b = H.permute3(db_up.reshape(1, k, D), (0, 2, 1)).reshape(D, k)
    # --- GRU layers, top layer first
    g_rnn = [None] * L
    dh_in = [None] * L
    for l in reversed(range(L)):
        dOut = dX.reshape(B, Fr, D)
        # W_hh^T (D, 3D): k-contiguous operand for the deep-ring backward kernel, straight
        # from the fp32 parameter (the same bf16 values as the forward's copy, no cast pass)
        WhhT = H.permute3(WhhF[l].detach().reshape(1, 3 * D, D), (0, 2, 1), dtype=T)
        dGH, dGHT, dGI, dGIT, bsum, ddir0 = _gru_layer_backward(
            T, B, D, Fr, dOut, gates[l], outs[l], h_in[l], Whh[l], WhhT)
        # dh_0 = dgh_0 . W_hh + dh_direct, as an NT product on W_hh^T (skinny ring path)
        dh_in[l] = H.gemm(dGHT[:, 0], WhhT, transB=True, M=B, N=D, K=3 * D,
                          lda=Fr * 3 * D, ldb=3 * D, cin=ddir0, beta=1.0)
        # previous hidden states of every step: [h_in, out[:, :F-1]] (written by the
        # persistent forward sweep when it ran, else built here)
        hprevT = hprevs[l]
        if hprevT is None:
            hprevT = torch.empty((B, Fr, D), device=dev, dtype=T)
            H.lib().call('srnn_copy2d', H.F32, H.dcode(T), B, D, H.ptr(h_in[l]), D,
                         H.ptr(hprevT), Fr * D, st())
            if Fr > 1:
                H.lib().call('srnn_copy2d', H.dcode(T), H.dcode(T), B, (Fr - 1) * D,
                             H.ptr(outsT[l]), Fr * D, H.ptr(hprevT[:, 1:]), Fr * D, st())
        dW_hh = H.gemm(dGHT.reshape(M, 3 * D), hprevT.reshape(M, D), transA=True)
        if bsum is not None:
            bs = H.colsum(bsum, B, 4 * D)               # sums of [dar | daz | dghn | dan]
            db_hh = bs[:3 * D]
            db_ih = torch.cat([bs[:2 * D], bs[3 * D:]])
            dGIT = dGIT.reshape(M, 3 * D)
        else:
            dGH2, dGI2 = dGH.reshape(M, 3 * D), dGI.reshape(M, 3 * D)
            db_hh = H.colsum(dGH2, M, 3 * D)
            dGIT = H.cast(dGI2, T)
            db_ih = H.colsum(dGI2, M, 3 * D)
        dW_ih = H.gemm(dGIT, xs[l], transA=True)
        dX = H.gemm(dGIT, Wih[l])                                     # (M, D)
        g_rnn[l] = [dW_ih, dW_hh, db_ih, db_hh]
    # --- input projections
    dx0 = dX
    dx0T = H.cast(dx0, T)
    dW_ie = H.gemm(dx0T, prevT, transA=True)                         # (D, nfs)
    g_ie = nn.weight_grad_to_params(mod.input_expand, dW_ie.reshape(D, nfs, 1))
    g_ie_b = H.colsum(dx0, M, D)
    d_upper = dx0.reshape(B, Fr, D) if ctx.has_upper else None
    if d_upper is not None and dx0T is not dx0:
        d_upper._srnn_lp = (dx0T, d_upper._version)     # (the upper tier's dY cast)
    grads = g_ie + [g_ie_b]
    if mod.is_cond:
        C = condT.shape[1]
        S = spk_embT.shape[1]
        dW_c = H.gemm(dx0T, condT, transA=True)                      # (D, C)
        grads += nn.weight_grad_to_params(mod.cond_expand, dW_c.reshape(D, C, 1))
        grads += [g_ie_b.clone()]                                    # cond bias grad
        dspk = torch.empty((B, D), device=dev, dtype=torch.float32)
        H.lib().call('srnn_segsum', H.ptr(dx0), D, B, Fr, D, H.ptr(dspk), st())
        dspkT = H.cast(dspk, T)
        dW_s = H.gemm(dspkT, spk_embT, transA=True)                  # (D, S)
        db_s = H.colsum(dspk, B, D)
        demb = H.gemm(dspkT, W_s)                                    # (B, S)
        dE = torch.zeros((S, S), device=dev, dtype=torch.float32)
        H.lib().call('srnn_index_add_rows', H.ptr(dE), S, S, H.ptr(spk_flat), B, S,
                     H.ptr(demb), S, st())
        grads += [dE]
        grads += nn.weight_grad_to_params(mod.spk_expand, dW_s.reshape(D, S, 1))
        grads += [db_s]
    for l in range(L):
        grads += g_rnn[l]
    grads += g_up + [g_up_b]
    dh0 = None
    if ctx.reset and need_h0:
        dh0 = torch.stack([H.colsum(dh_in[l], B, D) for l in range(L)], 0)
    return d_upper, dh0, grads


class SampleLevelMLP(torch.nn.Module):
    """model.py:266-325."""

    def __init__(self, frame_size, dim, q_levels, wnorm):
        super().__init__()
        self.q_levels = q_levels
        self.weight_norm = wnorm
        self.frame_size = frame_size
        self.dim = dim
        self.embedding = torch.nn.Embedding(q_levels, q_levels)
        self.input = torch.nn.Conv1d(q_levels, dim, kernel_size=frame_size, bias=False)
        init.kaiming_uniform_(self.input.weight)
        self.hidden = torch.nn.Conv1d(dim, dim, kernel_size=1)
        init.kaiming_uniform_(self.hidden.weight)
        init.constant_(self.hidden.bias, 0)
        self.output = torch.nn.Conv1d(dim, q_levels, kernel_size=1)
        nn.lecun_uniform(self.output.weight)
        init.constant_(self.output.bias, 0)
        if wnorm:
            nn.apply_weight_norm(self.input)
            nn.apply_weight_norm(self.hidden)
            nn.apply_weight_norm(self.output)

    def _param_list(self):
        return ([self.embedding.weight] + nn.weight_params(self.input) +
                nn.weight_params(self.hidden) + [self.hidden.bias] +
                nn.weight_params(self.output) + [self.output.bias])

    def tab(self, T):
        """Tab[k][q][:] = W_in[:, :, k] . E[q, :]  (FS0, Q, D): the folded embedding+conv."""
        return _build_tab(self, T)[0]

    def forward(self, prev_samples, upper_tier_conditioning):
        """model.py:308-325: indices (B, T+FS0-1), conditioning (B, T, D) -> log-probs (B,T,Q)."""
        H.need_cuda(upper_tier_conditioning)
        # (a window of the index stream is read in place: the kernels take a row stride)
        x = prev_samples.to(upper_tier_conditioning.device).long()
        if x.dim() != 2 or x.stride(1) != 1 or x.shape[1] != upper_tier_conditioning.shape[1] + \
                self.frame_size - 1:
            x = x.contiguous()
        u = upper_tier_conditioning
        if u.dtype not in (torch.float32, _dt(self)):
            u = u.float()
        # the registered op srnn::mlp_fwd (custom_ops.py; autograd: srnn::mlp_bwd)
        return custom_ops.mlp(x, u.contiguous(), self._param_list(), mlp_meta(self))


def _build_tab(mlp, T):
    Q, D, FS0 = mlp.q_levels, mlp.dim, mlp.frame_size
    W_in = nn.weight_of(mlp.input)                                       # (D, Q, FS0)
    Wp = H.permute3(W_in, (2, 0, 1), dtype=T)                            # (FS0, D, Q)
    ET = H.cast_param(mlp.embedding.weight, T)
    tab = torch.empty((FS0, Q, D), device=ET.device, dtype=T)
    H.gemm(ET, Wp, transB=True, out=tab, M=Q, N=D, K=Q, lda=Q, ldb=Q, ldc=D, batch=FS0, sA=0,
           sB=D * Q, sC=Q * D)
    return tab, Wp, ET


def mlp_forward(mlp, x, upper, ps):
    """SampleLevelMLP forward (model.py:308-325): (log-probs, state) (srnn::mlp_fwd)."""
    T = _dt(mlp)
    B, Tl, D = upper.shape
    Q, FS0 = mlp.q_levels, mlp.frame_size
    dev = upper.device
    tab, Wp, ET = _build_tab(mlp, T)
    a1 = torch.empty((B * Tl, D), device=dev, dtype=T)
    upper = upper.contiguous()
    # SRNN_MASK_BITS=1 (bf16): the ReLU masks of a1 and a2 leave the forward as bits, 16x
    # fewer bytes for the backward's masked GEMMs to read than the activations.  Off by
    # default: measured (MI355X, B = 128) the two masked dgrads gain 27 us each, but the
    # hidden GEMM's bit epilogue costs 26 us and the L1 gather's 2-B bit stores 87 us.
    bits = T == torch.bfloat16 and upper.dtype == T and D % 64 == 0 and \
        os.environ.get('SRNN_MASK_BITS', '0') != '0'
    # Default (bf16, D % 64 == 0): a1's mask alone leaves as bits, in the grouped layout
    # (u16 [D / 16][B T]): the da1 GEMM stages a tile's bits by LDS-DMA with its first
    # operand pieces instead of reading 2 B of a1 per output in its epilogue (SRNN_A1_BITS=0:
    # the bf16 mask).  The L1 kernel's 16-column workgroups write a column group's rows as
    # contiguous runs (the row-major layout's 2-B words of a row came from 64 workgroups).
    a1_bits = not bits and T == torch.bfloat16 and upper.dtype == T and D % 64 == 0 and \
        os.environ.get('SRNN_A1_BITS', '1') != '0'
    m1 = m2 = None
    ev = H.roof_begin()
    if bits:
        m1, m2 = H.relu_bits(B * Tl, D, dev), H.relu_bits(B * Tl, D, dev)
        H.lib().call('srnn_mlp_l1_bits', H.ptr(tab), H.ptr(x), x.stride(0), 0, B, Tl,
                     H.ptr(upper), D, H.ptr(a1), D, D, FS0, Q, H.ptr(m1), m1.stride(0),
                     H.stream())
    elif a1_bits:
        m1 = H.relu_bits_grouped(B * Tl, D, dev)
        H.lib().call('srnn_mlp_l1_bits', H.ptr(tab), H.ptr(x), x.stride(0), 0, B, Tl,
                     H.ptr(upper), D, H.ptr(a1), D, D, FS0, Q, H.ptr(m1), 0, H.stream())
    else:
        H.lib().call('srnn_mlp_l1', H.dcode(T), H.ptr(tab), H.ptr(x), x.stride(0), 0, B, Tl,
                     H.dcode(upper), H.ptr(upper), D, H.ptr(a1), D, D, FS0, Q, H.stream())
    # algorithmic bytes: upper read and a1 written once (+ its mask bits), the index windows
    H.roof_end('mlp_l1_gather', ev, B * Tl * D * (upper.element_size() + a1.element_size()) +
               (B * Tl * D // 8 if m1 is not None else 0) + B * (Tl + FS0 - 1) * 8)
    W_hid = _wcast(mlp.hidden, T).reshape(D, D)
    W_out = _wcast(mlp.output, T).reshape(Q, D)
    # bf16: the backward's activation-gradient GEMMs read W^T stored k-contiguous (the NT
    # shape of the pair-mode kernels: da1 1.43 -> 1.30 ms at B = 512, tools/da1_gemm_ab.py)
    W_t = (_wcast_t(mlp.hidden, T), _wcast_t(mlp.output, T)) if T == torch.bfloat16 else None
    ev = H.roof_begin()
    a2 = H.linear(a1, W_hid, bias=mlp.hidden.bias, relu=True, out_dtype=T, bits_out=m2)
    H.roof_end('mlp_hidden_gemm', ev, 2.0 * B * Tl * D * D)
    # bf16: the logits GEMM's epilogue applies the row log-softmax itself (its 256-column
    # tiles hold whole rows), so the (B T, Q) fp32 logits never round-trip through HBM
    # (SRNN_LSM_EPI=0: the separate logsoftmax pass)
    lsm = T == torch.bfloat16 and Q == 256 and os.environ.get('SRNN_LSM_EPI', '1') != '0'
    epi = H.GemmEpilogue(logsoftmax=True) if lsm else None
    z = H.linear(a2, W_out, bias=mlp.output.bias, epilogue=epi)      # (B*T, Q) fp32
    if lsm and epi.logsoftmax_served:
        logp = z
        _STATS['lsm_epi'] += 1
    else:
        logp = torch.empty((B * Tl, Q), device=dev, dtype=torch.float32)
        H.lib().call('srnn_logsoftmax_nll', H.ptr(z), Q, None, 0, Tl, B * Tl, Q, None,
                     H.ptr(logp), Q, None, H.F32, 0, 0.0, H.stream())
    ctx = _State()
    ctx.mlp = mlp
    ctx.T = T
    ctx.udt = upper.dtype
    ctx.dims = (B, Tl, D, Q, FS0)
    ctx.saved_tensors = (x, a1, a2, logp, Wp, ET, W_hid, W_out)
    ctx.bits = (m1, m2)
    ctx.W_t = W_t
    return logp.reshape(B, Tl, Q), ctx


def _mlp_out_bwd_unfused(T, M, D, Q, dz, a1, a2, m2, W_t, W_out, csum_epi):
    """The output layer's backward as separate calls (every dtype and shape): (dW_out, db_out,
    da2, dW_hid, db_hid)."""
    dev = dz.device
    dW_out = H.gemm(dz, a2, transA=True)                             # (Q, D)
    db_out = H.colsum(dz, M, Q)
    # (M, D) = dz . W_out, through W_out^T (D, Q) when the forward made it
    Wo, tB = (W_t[1], True) if W_t is not None else (W_out, False)
    # bf16: the da2 GEMM's epilogue also sums its stored columns per 128-row block (the
    # hidden layer's bias gradient) -- one pass over da2 fewer than a separate column sum
    csp = epi = None
    if csum_epi:
        csp = torch.empty((M // 128, D), device=dev, dtype=torch.float32)
        epi = H.GemmEpilogue(csum=csp)
    ev = H.roof_begin()
    if m2 is not None:
        da2 = H.gemm(dz, Wo, transB=tB, mask_bits=m2, out_dtype=T, epilogue=epi)
    else:
        da2 = H.gemm(dz, Wo, transB=tB, mask=a2, out_dtype=T, epilogue=epi)
    H.roof_end('mlp_da2_gemm', ev, 2.0 * M * D * Q)
    if csp is not None and not epi.csum_served:
        csp = None
    if csp is not None:
        _STATS['csum_epi'] += 1
    ev = H.roof_begin()
    dW_hid = H.gemm(da2, a1, transA=True)                            # (D, D)
    H.roof_end('mlp_dw_hid_gemm', ev, 2.0 * M * D * D)
    db_hid = H.colsum(csp, M // 128, D) if csp is not None else H.colsum(da2, M, D)
    return dW_out, db_out, da2, dW_hid, db_hid


def mlp_backward(ctx, dlogp, nll=None):
    """Backward of mlp_forward: (d_upper, [parameter gradients]).  nll = (target, T,
    gscale, g): the log-probs' gradient is sequence_nll_loss_bits' closed form (dlogp is then
    not read)."""
    mlp = ctx.mlp
    T = ctx.T
    B, Tl, D, Q, FS0 = ctx.dims
    x, a1, a2, logp, Wp, ET, W_hid, W_out = ctx.saved_tensors
    dev = logp.device
    st = H.stream
    M = B * Tl
    dz = torch.empty((M, Q), device=dev, dtype=T)
    if nll is not None:
        # loss gradient in closed form (custom_ops nll_bits): fused NLL + log-softmax
        # backward, dz = c (exp(logp) - onehot) straight into the GEMM operand dtype
        tg, Tt, gscale, gd = nll
        H.lib().call('srnn_nll_logsoftmax_bwd', H.ptr(tg), Tt, Tt, M, Q, H.ptr(logp), Q,
                     gscale, H.ptr(gd), H.ptr(dz), H.dcode(T), Q, st())
    else:
        dl = dlogp.reshape(M, Q).float().contiguous()
        H.lib().call('srnn_logsoftmax_bwd', H.ptr(dl), Q, H.ptr(logp), Q, M, Q, H.ptr(dz),
                     H.dcode(T), Q, st())
    m1, m2 = ctx.bits
    ctx.bits = None
    W_t = ctx.W_t
    ctx.W_t = None
    csum_epi = T == torch.bfloat16 and M % 256 == 0 and \
        os.environ.get('SRNN_CSUM_EPI', '1') != '0'
    # bf16: da2, dW_out and the hidden bias sums from ONE pass over dz and a2 (srnn_mlp_out_bwd;
    # the separate GEMMs fetch each of dz and a2 again).  The kernel keeps the separate calls'
    # summation orders, so every gradient keeps its bits; db_out stays the column pass over dz
    # (the kernel's own db_out sums in another order).  Shapes it does not serve (None) and
    # SRNN_OUT_BWD_FUSED=0 take the separate calls.  With a2's mask kept as bits
    # (SRNN_MASK_BITS=1) the kernel still masks by the a2 it stages for dW_out -- bit m2 is
    # a2 > 0 by construction: same bits (test_mask_bits_step_bf16 compares every gradient).
    fused = None
    if T == torch.bfloat16 and W_t is not None and os.environ.get('SRNN_OUT_BWD_FUSED', '1') != '0':
        ev = H.roof_begin()
        fused = H.mlp_out_bwd(dz, a2, W_t[1], want_db=False)
        if fused is not None:
            # (both products: da2 and dW_out)
            H.roof_end('mlp_da2_gemm', ev, 4.0 * M * D * Q)
    if fused is not None:
        da2, dW_out, _, csp = fused
        db_out = H.colsum(dz, M, Q)
        _STATS['out_bwd_fused'] += 1
        if csum_epi:
            _STATS['csum_epi'] += 1
            db_hid = H.colsum(csp, csp.shape[0], D)
        else:
            db_hid = H.colsum(da2, M, D)
        csp = None
        ev = H.roof_begin()
        dW_hid = H.gemm(da2, a1, transA=True)                        # (D, D)
        H.roof_end('mlp_dw_hid_gemm', ev, 2.0 * M * D * D)
    else:
        dW_out, db_out, da2, dW_hid, db_hid = _mlp_out_bwd_unfused(
            T, M, D, Q, dz, a1, a2, m2, W_t, W_out, csum_epi)
    # d(upper) in upper's dtype: bf16 when the bottom tier hands the MLP a bf16 upper.  A
    # bf16 da1 also gets max |da1| from the GEMM's epilogue (the packed dTab scatter's
    # scale), so the scatter needs no pass of its own over da1
    amax = blk = epi = None
    if ctx.udt == torch.bfloat16:
        amax = torch.zeros(1, device=dev, dtype=torch.int32)
        if FS0 == 16 and D % 256 == 0 and os.environ.get('SRNN_DTAB_BLK', '0') == '1':
            # ... and a column-blocked copy [D/4][M][4] of da1, the scatter's operand
            blk = torch.empty((D // 4, M, 4), device=dev, dtype=torch.bfloat16)
        epi = H.GemmEpilogue(amax=amax, blk=blk)
    Wh, tB = (W_t[0], True) if W_t is not None else (W_hid, False)
    ev = H.roof_begin()
    if m1 is not None:
        da1 = H.gemm(da2, Wh, transB=tB, mask_bits=m1, out_dtype=ctx.udt,     # (M, D)
                     epilogue=epi)
    else:
        da1 = H.gemm(da2, Wh, transB=tB, mask=a1, out_dtype=ctx.udt,          # (M, D)
                     epilogue=epi)
    H.roof_end('mlp_da1_gemm', ev, 2.0 * M * D * D)
    if epi is not None:
        if not epi.blk_served:
            blk = None
        if not epi.amax_served:
            amax = None
    # folded embedding . conv backward: dTab[q][k][:] += da1[t] for x_{t+k} = q
    dtabT = torch.empty((Q, FS0 * D), device=dev, dtype=T)
    work = torch.empty(H.mlp_dtab_plan(da1.dtype, T, B, Tl, D, FS0, Q).work_bytes // 8,
                       device=dev, dtype=torch.int64)
    # the same pass sums da1 over rows t = j (mod FS0): the bottom tier's upsampling bias
    # gradient (its output is this layer's `upper`), handed over on the returned gradient
    colsum = torch.empty(FS0 * D, device=dev, dtype=torch.float32)
    done = ctypes.c_int(0)
    ev = H.roof_begin()
    H.lib().call('srnn_mlp_dtab4', H.dcode(da1), H.ptr(da1), D, H.ptr(x), x.stride(0), 0, B,
                 Tl, H.ptr(dtabT), H.dcode(T), D, FS0, Q, H.ptr(work), work.numel() * 8,
                 H.ptr(colsum), ctypes.byref(done), H.ptr(amax), H.ptr(blk), st())
    blk = None
    # algorithmic bytes: da1 and the index window read once, dTab^T and the column sums
    # written once
    H.roof_end('dtab_scatter', ev, B * Tl * D * da1.element_size() +
               B * (Tl + FS0 - 1) * 8 + Q * FS0 * D * dtabT.element_size() + FS0 * D * 4)
    dE = H.gemm(dtabT, Wp.reshape(FS0 * D, Q))                       # (Q, Q)
    # dWp[k] = dTab[:, k]^T E for every tap k at once: (FS0 D, Q) = dtabT^T . ET, one GEMM
    # (the (FS0, D, Q) result is the same memory as the per-tap batch)
    dWp = torch.empty((FS0, D, Q), device=dev, dtype=torch.float32)
    H.gemm(dtabT, ET, transA=True, out=dWp, M=FS0 * D, N=Q, K=Q, lda=FS0 * D, ldb=Q, ldc=Q)
    dW_in = H.permute3(dWp, (1, 2, 0))                               # (D, Q, FS0)
    grads = [dE]
    grads += nn.weight_grad_to_params(mlp.input, dW_in)
    grads += nn.weight_grad_to_params(mlp.hidden, dW_hid.reshape(D, D, 1)) + [db_hid]
    grads += nn.weight_grad_to_params(mlp.output, dW_out.reshape(Q, D, 1)) + [db_out]
    d_upper = da1.reshape(B, Tl, D)
    if done.value:
        d_upper._srnn_colsum = (colsum, d_upper._version, FS0)
    return d_upper, grads


class Runner:
    """model.py:328-349."""

    def __init__(self, model):
        super().__init__()
        self.model = model
        self.reset_hidden_states()

    def reset_hidden_states(self):
        self.hidden_states = {rnn: None for rnn in self.model.frame_level_rnns}

    def run_rnn(self, rnn, prev_samples, upper_tier_conditioning, cond, spk, writer=None,
                iterations=None):
        (output, new_hidden) = rnn(prev_samples, upper_tier_conditioning,
                                   self.hidden_states[rnn], cond, spk, writer, iterations)
        self.hidden_states[rnn] = new_hidden.detach()    # TBPTT truncation (model.py:348)
        return output


class Predictor(Runner, torch.nn.Module):
    """model.py:352-436: teacher-forced forward with TBPTT hidden-state carry."""

    def __init__(self, model):
        super().__init__(model)

    def forward(self, input_sequences, reset, cond, spk, writer=None, iterations=None):
        if reset:
            self.reset_hidden_states()
        dev = next(self.model.parameters()).device
        H.need_cuda(torch.empty(0, device=dev))
        input_sequences = input_sequences.to(dev).long().contiguous()
        cond = cond.to(dev)
        spk = spk.to(dev)
        (batch_size, _) = input_sequences.size()
        (_, _, cond_dim) = cond.size()
        L = self.model.lookback
        q = self.model.q_levels
        mode = 0 if self.model.ulaw else 1
        upper = None
        for rnn in reversed(self.model.frame_level_rnns):
            n = rnn.n_frame_samples
            seg = input_sequences[:, L - n: input_sequences.shape[1] - n + 1]
            prev = utils._dequant(seg, q, 2.0, mode)                    # 2 * dequantize
            prev = prev.view(batch_size, -1, n)
            if upper is None:
                c = cond.contiguous().view(batch_size, -1, cond_dim)
                s = spk.contiguous().view(batch_size, -1)
                upper = self.run_rnn(rnn, prev, None, c, s, writer, iterations)
            else:
                upper = self.run_rnn(rnn, prev, upper, None, None, writer, iterations)
        fs0 = self.model.frame_level_rnns[0].frame_size
        return self.model.sample_level_mlp(input_sequences[:, L - fs0:], upper)


def generation_weights(model, dtype=None):
    """Folded, device-resident weight layouts for srnn::generate (weight-norm applied once):
    (tensors, meta) -- srnn_model_struct(tensors, meta) rebuilds the C ABI's SrnnModel."""
    T = dtype or model.compute_dtype
    D = model.dim
    ws = []
    meta = [len(model.frame_level_rnns), model.n_rnn, D, model.q_levels, model.cond_dim,
            H.dcode(T)]
    with torch.no_grad():
        for k, rnn in enumerate(model.frame_level_rnns):
            nfs = rnn.n_frame_samples
            W_ie = nn.weight_of(rnn.input_expand).reshape(D, nfs)
            if rnn.is_cond:
                C = model.cond_dim
                W_c = nn.weight_of(rnn.cond_expand).reshape(D, C)
                w_in = torch.empty((D, nfs + C), device=W_ie.device, dtype=T)
                H.lib().call('srnn_copy2d', H.F32, H.dcode(T), D, nfs, H.ptr(W_ie.contiguous()),
                             nfs, H.ptr(w_in), nfs + C, H.stream())
                H.lib().call('srnn_copy2d', H.F32, H.dcode(T), D, C, H.ptr(W_c.contiguous()), C,
                             H.ptr(w_in[:, nfs:]), nfs + C, H.stream())
                meta += [rnn.frame_size, nfs, nfs + C, 0]
                ws.append(w_in)
            else:
                meta += [rnn.frame_size, nfs, nfs, 1]
                ws += [H.cast(W_ie.contiguous(), T), rnn.input_expand.bias.detach().contiguous()]
            for l in range(model.n_rnn):
                ws += [H.cast(getattr(rnn.rnn, 'weight_ih_l%d' % l).detach().contiguous(), T),
                       H.cast(getattr(rnn.rnn, 'weight_hh_l%d' % l).detach().contiguous(), T),
                       getattr(rnn.rnn, 'bias_ih_l%d' % l).detach().contiguous(),
                       getattr(rnn.rnn, 'bias_hh_l%d' % l).detach().contiguous()]
            k_ = rnn.frame_size
            ws += [nn.convt_operand(rnn.upsampling.conv_t, T),
                   H.permute3(rnn.upsampling.bias.detach().reshape(1, D, k_), (0, 2, 1)),
                   rnn.h0.detach().float().contiguous()]
        mlp = model.sample_level_mlp
        ws += [mlp.tab(T), H.cast(nn.weight_of(mlp.hidden).reshape(D, D).contiguous(), T),
               mlp.hidden.bias.detach().contiguous(),
               H.cast(nn.weight_of(mlp.output).reshape(model.q_levels, D).contiguous(), T),
               mlp.output.bias.detach().contiguous()]
    meta.append(model.lookback)
    return ws, meta


def srnn_model_struct(ws, meta):
    """The C ABI's SrnnModel (include/samplernn_hip.h) over generation_weights' tensors."""
    m = H.SrnnModel()
    m.n_tiers, m.n_rnn, m.dim, m.q_levels, m.cond_dim, m.dtype = [int(v) for v in meta[:6]]
    it = iter(ws)
    for k in range(m.n_tiers):
        t = m.tier[k]
        t.frame_size, t.n_frame_samples, t.in_dim, has_b = [int(v) for v in
                                                            meta[6 + 4 * k: 10 + 4 * k]]
        t.w_in = H.ptr(next(it))
        if has_b:
            t.b_in = H.ptr(next(it))
        for l in range(m.n_rnn):
            t.w_ih[l], t.w_hh[l] = H.ptr(next(it)), H.ptr(next(it))
            t.b_ih[l], t.b_hh[l] = H.ptr(next(it)), H.ptr(next(it))
        t.w_up, t.b_up, t.h0 = H.ptr(next(it)), H.ptr(next(it)), H.ptr(next(it))
    m.tab, m.w_hid, m.b_hid = H.ptr(next(it)), H.ptr(next(it)), H.ptr(next(it))
    m.w_out, m.b_out = H.ptr(next(it)), H.ptr(next(it))
    return m


def top_row_bias(model, spk):
    """(n_seqs, D): spk_expand(spk_embedding(spk)) + b_spk + b_cond + b_in for the top tier."""
    top = model.frame_level_rnns[-1]
    D, S = model.dim, model.spk_dim
    dev = spk.device
    with torch.no_grad():
        n = spk.numel()
        emb = torch.empty((n, S), device=dev, dtype=torch.float32)
        H.lib().call('srnn_gather_rows', H.ptr(top.spk_embedding.weight), S,
                     H.ptr(spk.reshape(-1).contiguous()), n, S, H.ptr(emb), H.F32, S, H.stream())
        bias = torch.empty(D, device=dev, dtype=torch.float32)
        H.lib().call('srnn_axpby', H.ptr(bias), H.ptr(top.spk_expand.bias),
                     H.ptr(top.cond_expand.bias), 1.0, 1.0, D, H.stream())
        H.lib().call('srnn_axpby', H.ptr(bias), H.ptr(bias), H.ptr(top.input_expand.bias), 1.0,
                     1.0, D, H.stream())
        W_s = nn.weight_of(top.spk_expand).reshape(D, S).contiguous()
        return H.linear(emb, W_s, bias=bias)


def sampling_controls(n_seqs, temperature=1.0, top_k=0, q_levels=256):
    """Per-row sampling controls of Generator.__call__ as host tensors (a pure host function).

    temperature and top_k are scalars (broadcast to every row) or per-row sequences, arrays or
    tensors of length n_seqs.  temperature must be finite and >= 0 (0 = greedy, 1 = the model's
    own softmax); top_k an integer in [0, q_levels] (0 and q_levels both mean "off").  Returns
    None when every row is at the defaults (temperature 1, top-k off), else
    (temperature (n_seqs,) float32, top_k (n_seqs,) int32).  Raises ValueError otherwise."""
    def rows(v, name):
        a = v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)
        if a.dtype == object or a.dtype.kind not in 'biuf':
            raise ValueError('sampling_controls: %s must be numeric' % name)
        if a.ndim == 0:
            a = np.broadcast_to(a, (n_seqs,))
        if a.ndim != 1 or a.shape[0] != n_seqs:
            raise ValueError('sampling_controls: %s has shape %s, expected a scalar or (%d,)'
                             % (name, tuple(a.shape), n_seqs))
        return a
    t = rows(temperature, 'temperature').astype(np.float64)
    if not np.all(np.isfinite(t)) or np.any(t < 0):
        raise ValueError('sampling_controls: temperature must be finite and >= 0')
    k = rows(top_k, 'top_k')
    if k.dtype.kind == 'f':
        if not np.all(np.isfinite(k)) or np.any(k != np.round(k)):
            raise ValueError('sampling_controls: top_k must be integral')
    k = k.astype(np.int64)
    if np.any(k < 0) or np.any(k > q_levels):
        raise ValueError('sampling_controls: top_k must lie in [0, %d]' % q_levels)
    t32 = t.astype(np.float32)
    if np.all(t32 == 1.0) and np.all((k == 0) | (k == q_levels)):
        return None
    return torch.from_numpy(t32.copy()), torch.from_numpy(k.astype(np.int32))


def nucleus_control(n_seqs, top_p=1.0):
    """The per-row nucleus (top-p) control of Generator.__call__ as a host tensor (a pure host
    function, beside sampling_controls).

    top_p is a scalar (broadcast to every row) or a per-row sequence, array or tensor of length
    n_seqs; every value must be finite with 0 < p <= 1 (1 = off).  Returns None when every row
    is 1, else an (n_seqs,) float32 tensor.  Raises ValueError otherwise."""
    a = top_p.detach().cpu().numpy() if torch.is_tensor(top_p) else np.asarray(top_p)
    if a.dtype == object or a.dtype.kind not in 'biuf':
        raise ValueError('nucleus_control: top_p must be numeric')
    if a.ndim == 0:
        a = np.broadcast_to(a, (n_seqs,))
    if a.ndim != 1 or a.shape[0] != n_seqs:
        raise ValueError('nucleus_control: top_p has shape %s, expected a scalar or (%d,)'
                         % (tuple(a.shape), n_seqs))
    p32 = a.astype(np.float64).astype(np.float32)
    # (checked as the float32 the device reads: a p that rounds to 1 is off, one that rounds
    #  to 0 is out of the domain)
    if not np.all(np.isfinite(p32)) or np.any(p32 <= 0) or np.any(p32 > 1):
        raise ValueError('nucleus_control: top_p must be finite with 0 < top_p <= 1')
    if np.all(p32 == 1.0):
        return None
    return torch.from_numpy(p32.copy())


def stream_rows(n_seqs, stream_ids):
    """Generator.__call__'s stream_ids as a host tensor (a pure host function, beside
    sampling_controls): None, or an integer sequence, array or tensor of length n_seqs with every
    value in [0, 2^31) -- the Philox row of each local row (duplicates allowed: such rows draw the
    same noise).  Returns None or an (n_seqs,) int32 tensor.  Raises ValueError otherwise."""
    if stream_ids is None:
        return None
    a = (stream_ids.detach().cpu().numpy() if torch.is_tensor(stream_ids)
         else np.asarray(stream_ids))
    if a.dtype == object or a.dtype.kind not in 'iuf':
        raise ValueError('stream_rows: stream_ids must be integers')
    if a.ndim != 1 or a.shape[0] != n_seqs:
        raise ValueError('stream_rows: stream_ids has shape %s, expected (%d,)'
                         % (tuple(a.shape), n_seqs))
    if a.dtype.kind == 'f':
        if not np.all(np.isfinite(a)) or np.any(a != np.round(a)):
            raise ValueError('stream_rows: stream_ids must be integral')
        a = a.astype(np.float64)
    if np.any(a < 0) or np.any(a >= 2 ** 31):
        raise ValueError('stream_rows: stream_ids must lie in [0, 2^31)')
    return torch.from_numpy(a.astype(np.int32))


def serve_plan(lengths, slots, chunk_frames):
    """The calls by which Generator.serve runs requests of `lengths` conditioning frames through
    `slots` rows, at most chunk_frames frames per call (a pure host function).  Returns a list of
    (n, rows): n the call's frame count and rows, per slot, (request or None, f0, f1, fresh) --
    the slot generates frames [f0, f1) of the request, from a fresh record when `fresh`.
    The policy:
      * slot s starts with request s;
      * a call runs n = min(chunk_frames, largest remainder over the active slots) frames; an
        active slot produces min(n, remainder) of them (its row still runs n, on zero-padded
        conditioning: the surplus is trimmed and the row's state dropped);
      * after the call finished requests complete in slot order, then the free slots take the
        pending requests in request order, lowest slot first, each from a fresh record;
      * a slot with nothing to do carries a dummy row (None, 0, 0, True);
      * the plan ends when no slot is active."""
    lengths = [int(v) for v in lengths]
    slots, chunk_frames = int(slots), int(chunk_frames)
    if slots < 1 or chunk_frames < 1:
        raise ValueError('serve_plan: slots and chunk_frames must be >= 1')
    if any(v < 1 for v in lengths):
        raise ValueError('serve_plan: every request needs at least one frame')
    nxt = min(slots, len(lengths))
    req = [s if s < nxt else None for s in range(slots)]
    done = [0] * slots
    fresh = [True] * slots
    plan = []
    while any(r is not None for r in req):
        n = min(chunk_frames, max(lengths[r] - done[s] for s, r in enumerate(req)
                                  if r is not None))
        rows = []
        for s, r in enumerate(req):
            if r is None:
                rows.append((None, 0, 0, True))
                continue
            f1 = min(lengths[r], done[s] + n)
            rows.append((r, done[s], f1, fresh[s]))
            done[s], fresh[s] = f1, False
        plan.append((n, rows))
        for s, r in enumerate(req):
            if r is not None and done[s] == lengths[r]:
                req[s] = None
        for s in range(slots):
            if req[s] is None and nxt < len(lengths):
                req[s], done[s], fresh[s] = nxt, 0, True
                nxt += 1
    return plan


def gen_state_layout(meta):
    """[dtype, n_tiers, n_rnn, dim, lookback, row_bytes] of a GenState for generation_weights'
    meta under the process's fold switches."""
    import custom_ops
    return [int(meta[5]), int(meta[0]), int(meta[1]), int(meta[2]), int(meta[-1]),
            custom_ops.gen_state_row_bytes(meta)]


class GenState:
    """The recurrent state of n_seqs generation rows between two calls of Generator.__call__.

    blob    (n_seqs, row_bytes) uint8: one opaque record per row as srnn_generate5 writes it
            (header, last lookback samples, every tier's fp32 h, the folded ticks' carried
            products; include/samplernn_hip.h).  A record depends on its row's history only.
    layout  [dtype code, n_tiers, n_rnn, dim, lookback, row_bytes] the records were taken
            under; the library checks each record's own header when it is used.
    steps   (n_seqs,) int64 host tensor: generation steps each row has completed.
    """

    def __init__(self, blob, layout, steps):
        layout = [int(v) for v in layout]
        steps = torch.as_tensor(steps, dtype=torch.int64).reshape(-1).cpu()
        if (not torch.is_tensor(blob) or blob.dtype != torch.uint8 or blob.dim() != 2 or
                len(layout) != 6 or blob.shape[1] != layout[5] or
                steps.shape[0] != blob.shape[0]):
            raise ValueError('GenState: blob must be (n_seqs, row_bytes) uint8 with a 6-entry '
                             'layout and one step count per row')
        self.blob, self.layout, self.steps = blob, layout, steps

    n_seqs = property(lambda self: self.blob.shape[0])
    device = property(lambda self: self.blob.device)

    def rows(self, index):
        """The state of rows `index` (a sequence or tensor of row numbers, in that order:
        a permutation, a subset, or repeats to fork one row into several continuations)."""
        idx = torch.as_tensor(index, dtype=torch.long).reshape(-1).cpu()
        if idx.numel() == 0 or int(idx.min()) < 0 or int(idx.max()) >= self.n_seqs:
            raise IndexError('GenState.rows: row numbers must lie in [0, %d)' % self.n_seqs)
        return GenState(self.blob[idx.to(self.blob.device)].contiguous(), self.layout,
                        self.steps[idx].clone())

    @classmethod
    def cat(cls, states):
        """The rows of `states` (GenStates of one layout, on one device), one after another."""
        states = list(states)
        if not states or not all(isinstance(st, GenState) for st in states):
            raise ValueError('GenState.cat: a non-empty sequence of GenStates')
        for st in states[1:]:
            if st.layout != states[0].layout:
                raise ValueError('GenState.cat: layouts differ: %s and %s'
                                 % (states[0].layout, st.layout))
        return cls(torch.cat([st.blob for st in states]), states[0].layout,
                   torch.cat([st.steps for st in states]))

    def replace(self, index, other):
        """A new state whose rows `index` (distinct row numbers) are `other`'s rows, in order,
        step counts included; the rest are this state's."""
        idx = torch.as_tensor(index, dtype=torch.long).reshape(-1).cpu()
        if not isinstance(other, GenState) or other.layout != self.layout:
            raise ValueError('GenState.replace: the other state has another layout')
        if idx.numel() != other.n_seqs:
            raise ValueError('GenState.replace: %d row numbers for %d rows'
                             % (idx.numel(), other.n_seqs))
        if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= self.n_seqs):
            raise IndexError('GenState.replace: row numbers must lie in [0, %d)' % self.n_seqs)
        if idx.unique().numel() != idx.numel():
            raise ValueError('GenState.replace: row numbers must be distinct')
        blob, steps = self.blob.clone(), self.steps.clone()
        blob[idx.to(blob.device)] = other.blob.to(blob.device)
        steps[idx] = other.steps
        return GenState(blob, self.layout, steps)

    def to(self, device):
        return GenState(self.blob.to(device), self.layout, self.steps)

    def cpu(self):
        return self.to('cpu')

    def state_dict(self):
        """Plain tensors and ints (torch.save-able); from_state_dict rebuilds the state."""
        return {'blob': self.blob.detach().cpu().clone(), 'steps': self.steps.clone(),
                'layout': list(self.layout)}

    @classmethod
    def from_state_dict(cls, d, device=None):
        st = cls(d['blob'], d['layout'], d['steps'])
        return st.to(device) if device is not None else st


def forced_prefix(model, n_seqs, T, prefix, prefix_len):
    """Generator.__call__'s prefix / prefix_len as host tensors ((n_seqs, P) int64,
    (n_seqs,) int32 or None = all P), validated (a pure host function).  A floating-point
    prefix is a waveform: quantised with the model's own quantiser."""
    if prefix is None:
        if prefix_len is not None:
            raise ValueError('Generator: prefix_len given without a prefix')
        return None, None
    p = torch.as_tensor(np.asarray(prefix) if not torch.is_tensor(prefix) else prefix).cpu()
    if p.dim() == 1:
        p = p.unsqueeze(0).expand(n_seqs, -1)
    if p.dim() != 2 or p.shape[0] != n_seqs or p.shape[1] > T:
        raise ValueError('Generator: prefix has shape %s, expected (%d, <= %d)'
                         % (tuple(p.shape), n_seqs, T))
    Q = model.q_levels
    if p.dtype.is_floating_point:
        # (the quantiser maps a full-scale +1.0 to Q itself: held at the top level)
        p = (utils.uquantize if model.ulaw else utils.linear_quantize)(p.contiguous(), Q)
        p = p.clamp(0, Q - 1)
    elif p.dtype == torch.bool or p.dtype.is_complex:
        raise ValueError('Generator: prefix must hold sample indices or a float waveform')
    p = p.to(torch.int64).contiguous()
    P = p.shape[1]
    if P and (int(p.min()) < 0 or int(p.max()) >= Q):
        raise ValueError('Generator: prefix indices must lie in [0, %d)' % Q)
    if prefix_len is None:
        return p, None
    a = (prefix_len.detach().cpu().numpy() if torch.is_tensor(prefix_len)
         else np.asarray(prefix_len))
    if a.dtype == object or a.dtype.kind not in 'iu':
        raise ValueError('Generator: prefix_len must be integral')
    if a.ndim == 0:
        a = np.broadcast_to(a, (n_seqs,))
    if a.ndim != 1 or a.shape[0] != n_seqs:
        raise ValueError('Generator: prefix_len has shape %s, expected a scalar or (%d,)'
                         % (tuple(a.shape), n_seqs))
    a = a.astype(np.int64)
    if np.any(a < 0) or np.any(a > P):
        raise ValueError('Generator: prefix_len must lie in [0, %d]' % P)
    return p, torch.from_numpy(a.astype(np.int32))


def bits_per_sample(scores, lengths=None):
    """Bits per sample of scored audio: -mean(scores[..., 0]) / ln 2 per row, for the (n_seqs, T,
    2) scores of Generator.score or of a return_scores call (a (T, 2) array is one row).
    lengths: the rows' own sample counts (a scalar or one per row, in [1, T]); the mean is then
    over each row's first lengths[b] steps.  Accumulated in float64; returns a float64 (n_seqs,)
    tensor (a pure host function)."""
    sc = torch.as_tensor(np.asarray(scores) if not torch.is_tensor(scores) else scores)
    sc = sc.detach().cpu()
    if sc.dim() == 2:
        sc = sc.unsqueeze(0)
    if sc.dim() != 3 or sc.shape[2] != 2 or sc.shape[1] < 1:
        raise ValueError('bits_per_sample: scores must be (n_seqs, T >= 1, 2), got %s'
                         % (tuple(sc.shape),))
    n, T = sc.shape[0], sc.shape[1]
    lp = sc[..., 0].to(torch.float64)
    if lengths is None:
        return -lp.mean(1) / math.log(2.0)
    ln = torch.as_tensor(lengths).reshape(-1).to(torch.int64)
    if ln.numel() == 1:
        ln = ln.expand(n)
    if ln.numel() != n or int(ln.min()) < 1 or int(ln.max()) > T:
        raise ValueError('bits_per_sample: lengths must be a scalar or (%d,) values in [1, %d]'
                         % (n, T))
    keep = torch.arange(T).unsqueeze(0) < ln.unsqueeze(1)
    return -(lp * keep).sum(1) / ln.to(torch.float64) / math.log(2.0)


def session_chunk_check(level, max_frames, frames, have_spk, temperature=None, top_k=None,
                        top_p=None, prefix=None):
    """What GenSession.chunk refuses before anything runs (a pure host function; the library
    makes the same checks): `frames` outside [1, max_frames], a control or a prefix above the
    session's `level` (temperature / top_k / prefix need 1, top_p needs 2), no spk on the first
    chunk (have_spk: an earlier chunk gave one, or this one does).  Raises ValueError."""
    if not 1 <= int(frames) <= int(max_frames):
        raise ValueError('GenSession.chunk: %d frames, the session was opened for 1..%d'
                         % (frames, max_frames))
    need = 2 if top_p is not None else 1 if (temperature is not None or top_k is not None or
                                             prefix is not None) else 0
    if need > level:
        raise ValueError('GenSession.chunk: %s needs a session of level >= %d, this one is of '
                         'level %d' % ('top_p' if need == 2 else 'temperature / top_k / a prefix',
                                       need, level))
    if not have_spk:
        raise ValueError('GenSession.chunk: the first chunk must give spk')


def session_advance(steps, frames, lookback, philox=True):
    """The host mirror of a session's per-row step counts after a chunk of `frames` frames (a
    pure host function): steps + frames * lookback, an int64 tensor.  Under device noise
    (philox) a row whose count would pass the 32-bit Philox step counter raises ValueError, as
    the library refuses the chunk."""
    steps = torch.as_tensor(steps, dtype=torch.int64).reshape(-1)
    T = int(frames) * int(lookback)
    if philox and steps.numel() and int(steps.max()) + T > 0xFFFFFFFF:
        b = int(steps.argmax())
        raise ValueError('GenSession.chunk: row %d: step0 %d + %d steps overflow the 32-bit '
                         'Philox step counter' % (b, int(steps[b]), T))
    return steps + T


class GenSession:
    """A generation session (Generator.session; srnn_gen_session_*): consecutive chunks of one
    (model, n_seqs, control level, switches) without a call's set-up.  The generation weight
    layouts, the folded tick weights, the workspace, the rows' records and the captured blocks
    are made once and kept; a chunk copies its inputs in, runs and copies its samples out.

    A session SNAPSHOTS generation_weights(model) when it is opened: later updates of the
    model's parameters are not seen (open a new session after training steps).  The speaker
    embedding behind `spk` is the exception: it is read from the model by each chunk that gives
    spk.  What a chunk generates is what the Generator.__call__ with state=<the session's
    state>, stream_ids=<the rows' ids> and the same inputs generates, bit for bit.

    scores=True opens the session for score pairs (level 3: every control and a forced prefix
    allowed; the arena grows by 8 bytes per row-step): chunk_scored(...) is then chunk(...)
    with the chunk's host float32 (n_seqs, T, 2) scores (Generator.__call__'s) appended.

    steps   (n_seqs,) int64 host tensor: the steps each row has completed.
    last_sequences   the last chunk's sample indices, (n_seqs, frames * lookback) on the device.
    Use after close() raises RuntimeError; a session is a context manager."""

    def __init__(self, generator, n_seqs, max_frames, dtype=None, level=0, seed=0,
                 persistent=True, use_graph=True, return_logp=False, replay_noise=False,
                 row_offset=0, scores=False):
        import custom_ops
        model = generator.model
        self.model = model
        self.n_seqs, self.max_frames, self.level = int(n_seqs), int(max_frames), int(level)
        if self.level not in (0, 1, 2):
            raise ValueError('GenSession: level must be 0, 1 or 2 (scores=True opens the scored '
                             'level)')
        self.scores = bool(scores)
        if self.scores:
            self.level = 3               # (the scored builds carry every control)
        self.return_logp, self.replay_noise = bool(return_logp), bool(replay_noise)
        self._dev = next(model.parameters()).device
        H.need_cuda(torch.empty(0, device=self._dev))
        self._handle = None
        self.weights, self.meta = generation_weights(model, dtype)
        flags = ((H.GEN_SESSION_GRAPH if use_graph else 0) |
                 (0 if persistent else H.GEN_SESSION_PER_SAMPLE) |
                 (H.GEN_SESSION_LOGP if return_logp else 0) |
                 (H.GEN_SESSION_NOISE if replay_noise else 0) |
                 (H.GEN_SESSION_SCORE if self.scores else 0))
        with torch.no_grad():
            self._handle, self._arena = custom_ops.gen_session_open(
                self.weights, self.meta, self.n_seqs, self.max_frames, self.level, seed,
                row_offset, flags)
        self.steps = torch.zeros(self.n_seqs, dtype=torch.int64)
        self.last_sequences = None
        self._have_spk = False
        self._ctl = [1.0, 0, 1.0]            # temperature, top_k, top_p of the previous chunk

    def _live(self):
        if self._handle is None:
            raise RuntimeError('GenSession: the session is closed')
        return self._handle

    def chunk(self, cond, spk=None, temperature=None, top_k=None, top_p=None, prefix=None,
              prefix_len=None, stream_ids=None, noise=None):
        """Generates cond's frames ((frames, C) shared or (n_seqs, frames, C), at most
        max_frames) from where the rows stand, and returns what Generator.__call__ returns:
        host float32 (n_seqs, frames * lookback) samples, with return_logp (samples, log-probs
        (n_seqs, T, Q)).  spk, temperature, top_k, top_p and stream_ids at None stay as in the
        previous chunk (at first: required, 1, off, 1, row_offset + b); prefix / prefix_len
        force this chunk only.  noise: this chunk's (T, n_seqs, Q) Exp(1) draws, given exactly
        when the session was opened with replay_noise."""
        return self._chunk(False, cond, spk, temperature, top_k, top_p, prefix, prefix_len,
                           stream_ids, noise)

    def chunk_scored(self, cond, spk=None, temperature=None, top_k=None, top_p=None, prefix=None,
                     prefix_len=None, stream_ids=None, noise=None):
        """chunk(...) with the chunk's host float32 (n_seqs, T, 2) score pairs appended (last).
        Only on a session opened with scores=True: ValueError otherwise, before anything runs
        (the library makes the same check before it queues anything)."""
        return self._chunk(True, cond, spk, temperature, top_k, top_p, prefix, prefix_len,
                           stream_ids, noise)

    def _chunk(self, return_scores, cond, spk, temperature, top_k, top_p, prefix, prefix_len,
               stream_ids, noise):
        handle = self._live()
        if return_scores and not self.scores:
            raise ValueError('GenSession.chunk_scored: scores need a session opened with '
                             'scores=True')
        model, n_seqs, dev = self.model, self.n_seqs, self._dev
        cond = torch.as_tensor(np.asarray(cond) if not torch.is_tensor(cond) else cond)
        if cond.dim() == 2:
            cond = cond.unsqueeze(0).expand(n_seqs, *cond.shape)
        if cond.dim() != 3 or cond.shape[0] != n_seqs:
            raise ValueError('GenSession.chunk: cond must be (frames, C) or (%d, frames, C)'
                             % n_seqs)
        frames = cond.shape[1]
        session_chunk_check(self.level, self.max_frames, frames,
                            self._have_spk or spk is not None, temperature, top_k, top_p, prefix)
        L, Q = model.lookback, model.q_levels
        T = frames * L
        if (noise is not None) != self.replay_noise:
            raise ValueError('GenSession.chunk: noise is given by exactly the chunks of a '
                             'session opened with replay_noise=True')
        steps = session_advance(self.steps, frames, L, not self.replay_noise)
        row_bias = None
        if spk is not None:
            spk = torch.as_tensor(np.asarray(spk) if not torch.is_tensor(spk) else spk).reshape(-1)
            if spk.numel() == 1:
                spk = spk.expand(n_seqs)
            row_bias = top_row_bias(model, spk.to(dev, torch.long).contiguous())
        tau = k = p = None
        if temperature is not None or top_k is not None:
            ctl = [self._ctl[0] if temperature is None else temperature,
                   self._ctl[1] if top_k is None else top_k]
            got = sampling_controls(n_seqs, ctl[0], ctl[1], Q)
            tau, k = got if got is not None else (torch.ones(n_seqs, dtype=torch.float32),
                                                  torch.zeros(n_seqs, dtype=torch.int32))
            self._ctl[:2] = ctl
        if top_p is not None:
            p = nucleus_control(n_seqs, top_p)
            p = p if p is not None else torch.ones(n_seqs, dtype=torch.float32)
            self._ctl[2] = top_p
        prefix, prefix_len = forced_prefix(model, n_seqs, T, prefix, prefix_len)
        if prefix is not None and prefix.shape[1] == 0:
            prefix = prefix_len = None
        ids = stream_rows(n_seqs, stream_ids)
        if noise is not None:
            noise = torch.as_tensor(noise).to(dev, torch.float32).contiguous()
            if noise.shape != (T, n_seqs, Q):
                raise ValueError('GenSession.chunk: noise must be (T, n_seqs, Q)')
        on = (lambda t: None if t is None else t.to(dev))
        with torch.no_grad():
            args = (handle, L, cond.to(dev, torch.float32).contiguous(), row_bias, on(tau), on(k),
                    on(p), on(prefix), on(prefix_len), ids, noise, self.return_logp)
            if return_scores:
                seq, logp, score = torch.ops.srnn.gen_session_chunk_scored(*args)
            else:
                seq, logp = torch.ops.srnn.gen_session_chunk(*args)
        self.steps = steps
        self._have_spk = True
        self.last_sequences = seq
        res = (model.dequantize(seq, Q).cpu(),)
        if self.return_logp:
            res += (logp.permute(1, 0, 2).contiguous(),)
        if return_scores:
            res += (score.permute(1, 0, 2).contiguous().cpu(),)
        return res if len(res) > 1 else res[0]

    def state(self):
        """The rows' GenState after the chunks so far (a copy: the session keeps its own)."""
        layout = gen_state_layout(self.meta)
        blob = torch.ops.srnn.gen_session_state(self._live(), self.weights[0], self.n_seqs,
                                                layout[5])
        return GenState(blob, layout, self.steps.clone())

    def replace(self, rows, state):
        """Rows `rows` (distinct row numbers) continue from `state`'s rows, in order, step
        counts included -- fresh_state() records start new streams there.  The library checks
        every record's header against the session's layout before it writes any."""
        import custom_ops
        handle = self._live()
        idx = torch.as_tensor(rows, dtype=torch.long).reshape(-1).cpu()
        if not isinstance(state, GenState):
            raise TypeError('GenSession.replace: state must be a GenState')
        if idx.numel() != state.n_seqs or idx.numel() == 0:
            raise ValueError('GenSession.replace: %d row numbers for %d rows'
                             % (idx.numel(), state.n_seqs))
        if int(idx.min()) < 0 or int(idx.max()) >= self.n_seqs:
            raise IndexError('GenSession.replace: row numbers must lie in [0, %d)' % self.n_seqs)
        if idx.unique().numel() != idx.numel():
            raise ValueError('GenSession.replace: row numbers must be distinct')
        custom_ops.gen_session_replace(handle, idx.to(torch.int32).contiguous(),
                                       state.blob.to(self._dev))
        self.steps = self.steps.clone()
        self.steps[idx] = state.steps

    def stats(self):
        """{'prepares', 'graphs_captured', 'graph_launches', 'eager_blocks', 'chunks',
        'steps_min', 'steps_max'}: the library's diagnostic counters of this session."""
        import custom_ops
        return custom_ops.gen_session_stats(self._live())

    def close(self):
        """Drains the session and releases it; further use raises.  Closing twice is allowed."""
        import custom_ops
        if self._handle is not None:
            handle, self._handle = self._handle, None
            try:
                custom_ops.gen_session_close(handle)
            finally:
                self._arena = self.weights = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Generator(Runner):
    """model.py:439-520: autoregressive generation, the whole loop on the device.

    __call__(n_seqs, seq_len, cond, spk) keeps the reference contract: `seq_len` is
    ignored (recomputed as num_cond * lookback, model.py:455), `cond` is a (num_cond, C)
    array shared by all rows (or (n_seqs, num_cond, C) per row), `spk` an int (or one per
    row), and the result is a host float32 (n_seqs, num_cond * lookback) tensor of
    dequantized samples.  Sampling is argmax(p / q), q ~ Exp(1), exactly what torch>=2's
    CPU `multinomial(1)` computes: sampler='torch' draws q from torch's CPU generator in
    the reference's order (bit-replay of the reference stream); sampler='philox' draws q
    on the device (counter-based Philox4x32-10, seed) for long runs.  `cuda` is accepted
    for API compatibility; the product path always runs on the GPU.  persistent=True (the
    default) runs the sample chain between bottom-tier ticks as one persistent launch
    (gen_mlp.hip) where the shape fits, else per-sample kernels.

    temperature / top_k (not in the reference; scalars or one value per row, see
    sampling_controls) change the draw inside the same launches: over the top_k largest
    logits of the row (ties at the k-th kept; 0 = all), argmax(z - temperature log q), and
    plain argmax z at temperature 0 (greedy; the noise is unused).  The noise each (row, step)
    consumes is unchanged, so a row at the defaults inside a mixed batch reproduces its
    uncontrolled stream.  With return_logp the log-probs stay the model's own log-softmax of
    the logits, NOT the tempered or truncated distribution that was drawn from.

    top_p (nucleus_control: a scalar or one value per row, 0 < p <= 1, 1 = off) cuts the draw
    further, to the smallest set of most probable classes of the top-k set whose tempered mass
    exp((z - max z) / temperature), renormalised over that set, reaches top_p: the class that
    crosses top_p is included and ties at the cut are kept.  Greedy rows ignore it.

    Streaming (not in the reference).  return_state=True appends a GenState to the result: the
    rows' recurrent state after the call.  state=<GenState> starts the call from it in place of
    h0 and the q_zero history, with `cond` holding the NEXT frames: an utterance generated as
    consecutive calls over slices of cond (and of `noise`, when replayed) equals the single
    call bit for bit, indices and log-probs.  Under sampler='philox' the device noise continues
    from the state's step count, which must then be the same for every row (ValueError);
    replayed noise has no such constraint.  prefix ((n_seqs, P) indices, or a float waveform
    quantised with the model's quantiser; P <= T) with prefix_len (a scalar or one value per
    row in [0, P]; default P) forces row b's first prefix_len[b] steps to the given samples:
    log-probs are still reported and noise still consumed at those steps, and a forced step
    overrides temperature, top_k and top_p.  stream() yields an utterance chunk by chunk,
    prime() returns the state after given audio.

    Continuous batching (not in the reference).  stream_ids (stream_rows: one integer in
    [0, 2^31) per row) names the Philox row of each local row in place of row_offset + b, and
    under sampler='philox' every row then draws from its own state.steps[b] on, so the rows of
    `state` may be at differing step counts: a stream keeps its noise whichever row serves it
    and whatever its neighbours are doing.  With replayed noise stream_ids has no effect.
    fresh_state() returns records of rows that have done no step (a call from them is the call
    from state=None), GenState.cat / replace join states, and serve() runs requests of differing
    lengths through a fixed number of rows (serve_plan states the policy).

    Scores (not in the reference).  return_scores=True appends a host float32 (n_seqs, T, 2)
    tensor: [..., 0] the log-prob of each step's sample -- the one drawn, or the given one at a
    forced step; the dense logp gathered there, bit for bit -- and [..., 1] the entropy of the
    model's softmax at that step, in nats.  Both describe the model's own distribution whatever
    the controls did to the draw.  8 bytes per row-step where return_logp takes 1 KiB; the index
    stream is the unscored call's.  score() scores given audio (every step forced),
    bits_per_sample() reduces scores to bits per sample; stream, serve and session pass scores
    through.
    """

    def __init__(self, model, cuda=False):
        super().__init__(model)
        self.cuda = cuda
        self.last_sequences = None
        self.last_state = None
        self.last_serve = None

    def __call__(self, n_seqs, seq_len, cond, spk, sampler='torch', seed=0, noise=None,
                 return_logp=False, use_graph=True, dtype=None, persistent=True, row_offset=0,
                 temperature=1.0, top_k=0, top_p=1.0, state=None, return_state=False,
                 prefix=None, prefix_len=None, stream_ids=None, controls_level=0,
                 return_scores=False):
        """row_offset: these n_seqs rows are rows [row_offset, row_offset + n_seqs) of a larger
        batch (rank-sharded generation, see shard_generate): the Philox noise (sampler='philox')
        is that of the global rows, so shards reproduce the single-process stream.
        temperature, top_k, top_p: the sampling controls (class docstring); at their defaults
        the call is the uncontrolled one, op and kernels, and with top_p at 1 it is the call
        without top_p.  return_logp's log-probs are the model's
        log-softmax whatever the controls.
        state, return_state, prefix, prefix_len: streaming (class docstring); at their defaults
        the call launches exactly what it launches without them.
        stream_ids: the rows' Philox rows and, with `state`, their own step origins (class
        docstring); None: nothing changes.  controls_level: 1 / 2 passes the control arrays of
        that level even where every row is at its defaults (serve: one build for all calls).
        return_scores: appends the (n_seqs, T, 2) scores (class docstring) after logp and before
        the state; at False the call launches exactly what it launches without it."""
        model = self.model
        self.reset_hidden_states()
        dev = next(model.parameters()).device
        H.need_cuda(torch.empty(0, device=dev))
        cond = torch.as_tensor(np.asarray(cond) if not torch.is_tensor(cond) else cond)
        if cond.dim() == 2:
            cond = cond.unsqueeze(0).expand(n_seqs, *cond.shape)
        cond = cond.to(dev, torch.float32).contiguous()
        num_cond = cond.shape[1]
        spk = torch.as_tensor(np.asarray(spk) if not torch.is_tensor(spk) else spk).reshape(-1)
        if spk.numel() == 1:
            spk = spk.expand(n_seqs)
        spk = spk.to(dev, torch.long).contiguous()
        L = model.lookback
        T = num_cond * L
        Q = model.q_levels
        ctrl = sampling_controls(n_seqs, temperature, top_k, Q)
        nucleus = nucleus_control(n_seqs, top_p)
        ids = stream_rows(n_seqs, stream_ids)
        if controls_level >= 2 and nucleus is None:
            nucleus = torch.ones(n_seqs, dtype=torch.float32)
        if (nucleus is not None or controls_level >= 1) and ctrl is None:
            ctrl = (torch.ones(n_seqs, dtype=torch.float32), torch.zeros(n_seqs, dtype=torch.int32))
        weights, meta = generation_weights(model, dtype)
        row_bias = top_row_bias(model, spk)
        if noise is None and sampler == 'torch':
            noise = torch.empty(T, n_seqs, Q).exponential_(1)
        if noise is not None:
            noise = torch.as_tensor(noise).to(dev, torch.float32).contiguous()
            assert noise.shape == (T, n_seqs, Q), 'noise must be (T, n_seqs, Q)'
        # the registered op srnn::generate (custom_ops.py): the whole sample loop on the device
        # (with sampling controls: srnn::generate_ctrl, the same loop with them in the draw)
        philox = noise is None
        if not philox:
            ids = None                   # (replayed noise: indexed by the call's own rows)
        streaming = (state is not None or return_state or prefix is not None or
                     prefix_len is not None or ids is not None)
        score = None
        if streaming or return_scores:
            state_blob, step0 = self._stream_state(state, n_seqs, dev, philox and ids is None)
            prefix, prefix_len = forced_prefix(model, n_seqs, T, prefix, prefix_len)
        with torch.no_grad():
            args = (weights, meta, cond, row_bias, noise, int(seed) & ((1 << 63) - 1),
                    int(row_offset), (1 if use_graph else 0) | (0 if persistent else 2),
                    bool(return_logp))
            if streaming or return_scores:
                # srnn::generate_stream: the same loop from a carried state and / or along a
                # forced prefix (srnn_generate5); controls at their defaults stay None
                sargs = args + (
                    ctrl[0].to(dev) if ctrl is not None else None,
                    ctrl[1].to(dev) if ctrl is not None else None,
                    nucleus.to(dev) if nucleus is not None else None, state_blob, step0,
                    prefix.to(dev) if prefix is not None else None,
                    prefix_len.to(dev) if prefix_len is not None else None, bool(return_state))
                if return_scores:
                    # srnn::generate_scored: the scored builds, every other input as it is
                    # (srnn_generate7)
                    seq, logp, blob, score = torch.ops.srnn.generate_scored(
                        *sargs, ids.to(dev) if ids is not None else None,
                        state.steps.to(dev) if state is not None and ids is not None else None)
                elif ids is None:
                    seq, logp, blob = torch.ops.srnn.generate_stream(*sargs)
                else:
                    # srnn::generate_rows: with the rows' own Philox origins (srnn_generate6)
                    seq, logp, blob = torch.ops.srnn.generate_rows(
                        *sargs, ids.to(dev), state.steps.to(dev) if state is not None else None)
            elif ctrl is None:
                seq, logp = torch.ops.srnn.generate(*args)
            elif nucleus is not None:
                seq, logp = torch.ops.srnn.generate_ctrl_p(*args, ctrl[0].to(dev), ctrl[1].to(dev),
                                                           nucleus.to(dev))
            else:
                seq, logp = torch.ops.srnn.generate_ctrl(*args, ctrl[0].to(dev), ctrl[1].to(dev))
        assert utils.q_zero(Q) == Q // 2
        self.last_sequences = seq
        out = model.dequantize(seq[:, L:], Q).cpu()
        res = (out,)
        if return_logp:
            res += (logp.permute(1, 0, 2).contiguous(),)
        if return_scores:
            res += (score.permute(1, 0, 2).contiguous().cpu(),)
        if return_state:
            before = state.steps if state is not None else torch.zeros(n_seqs, dtype=torch.int64)
            res += (GenState(blob, gen_state_layout(meta), before + T),)
        return res if len(res) > 1 else out

    def score(self, samples, cond, spk, dtype=None, chunk_frames=0):
        """Scores given audio under the generation path: `samples` ((n_seqs, T) indices, or a
        float waveform quantised with the model's quantiser, as prefix= accepts; T = num_cond *
        lookback exactly) is forced at every step, and the result is the host float32
        (n_seqs, T, 2) scores of __call__(prefix=samples, return_scores=True): the log-prob of
        each given sample and the model's entropy there (bits_per_sample reduces them).  With
        chunk_frames > 0 the audio is scored chunk_frames conditioning frames at a time, each
        call continuing from the last one's state -- the same scores bit for bit, in memory
        bounded by the chunk."""
        x = torch.as_tensor(np.asarray(samples) if not torch.is_tensor(samples) else samples)
        if x.dim() == 1:
            x = x.unsqueeze(0)
        cond = torch.as_tensor(np.asarray(cond) if not torch.is_tensor(cond) else cond)
        fdim = cond.dim() - 2
        num_cond, L = cond.shape[fdim], self.model.lookback
        if x.dim() != 2 or x.shape[1] != num_cond * L:
            raise ValueError('Generator.score: samples of shape %s, expected (n_seqs, %d) = '
                             'num_cond * lookback samples' % (tuple(x.shape), num_cond * L))
        n_seqs = x.shape[0]
        chunk_frames = int(chunk_frames)
        if chunk_frames < 0:
            raise ValueError('Generator.score: chunk_frames must be >= 0')
        # (every step is forced: no noise is needed)
        kw = dict(sampler='philox', dtype=dtype, return_scores=True)
        if chunk_frames == 0 or chunk_frames >= num_cond:
            return self(n_seqs, 0, cond, spk, prefix=x, **kw)[-1]
        parts, state = [], None
        for f0 in range(0, num_cond, chunk_frames):
            f1 = min(num_cond, f0 + chunk_frames)
            _, sc, state = self(n_seqs, 0, cond.narrow(fdim, f0, f1 - f0), spk, state=state,
                                return_state=True, prefix=x[:, f0 * L:f1 * L], **kw)
            parts.append(sc)
        self.last_state = state
        return torch.cat(parts, 1)

    @staticmethod
    def _stream_state(state, n_seqs, dev, philox):
        """(records on the device or None, step0) of a call that continues `state`."""
        if state is None:
            return None, 0
        if not isinstance(state, GenState):
            raise TypeError('Generator: state must be a GenState')
        if state.n_seqs != n_seqs:
            raise ValueError('Generator: state holds %d rows, the call has %d'
                             % (state.n_seqs, n_seqs))
        step0 = 0
        if philox:      # (and no stream_ids: with them every row has its own origin)
            # one step origin per call: the device noise of step t is Philox(row, step0 + t)
            if bool((state.steps != state.steps[0]).any()):
                raise ValueError('Generator: rows at differing step counts %s cannot continue '
                                 'under sampler=\'philox\' (replayed noise can)'
                                 % sorted(set(state.steps.tolist())))
            step0 = int(state.steps[0])
        return state.blob.to(dev), step0

    def fresh_state(self, n_seqs, dtype=None):
        """The GenState of n_seqs rows that have done no step (srnn::gen_state_fresh): h0, the
        q_zero history and, with folded ticks, their carried products as a fresh start of n_seqs
        rows computes them.  A call with state=fresh_state(n_seqs) equals the call with
        state=None bit for bit, and every row of the result is the same record."""
        n_seqs = int(n_seqs)
        dev = next(self.model.parameters()).device
        H.need_cuda(torch.empty(0, device=dev))
        weights, meta = generation_weights(self.model, dtype)
        with torch.no_grad():
            blob = torch.ops.srnn.gen_state_fresh(weights, meta, n_seqs)
        return GenState(blob, gen_state_layout(meta), torch.zeros(n_seqs, dtype=torch.int64))

    def session(self, n_seqs, max_frames, dtype=None, level=0, seed=0, persistent=True,
                use_graph=True, return_logp=False, replay_noise=False, row_offset=0,
                scores=False):
        """A GenSession of n_seqs rows for chunks of at most max_frames conditioning frames:
        the generation weights (SNAPSHOT here: later parameter updates are not seen), the
        workspace, the rows' records -- fresh ones -- and the captured blocks are kept between
        its chunks.  level: the sampling controls its chunks may carry (0 none, 1 temperature /
        top_k / prefix, 2 with top_p); seed: the Philox seed of every chunk; replay_noise: every
        chunk brings its noise (sampler='torch' streams), else the device draws it;
        row_offset: the Philox row of row b is row_offset + b until a chunk gives stream_ids.
        dtype, persistent, use_graph, return_logp: as in __call__.  scores: its chunks may
        return score pairs (GenSession.chunk_scored)."""
        return GenSession(self, n_seqs, max_frames, dtype, level, seed, persistent, use_graph,
                          return_logp, replay_noise, row_offset, scores)

    def serve(self, requests, slots, chunk_frames, seed=0, dtype=None, persistent=True,
              use_graph=True, session=False, scores=False):
        """Continuous batching: runs `requests` -- dicts with cond (F_u, C) and spk, optionally
        stream_id (default: the request's position), temperature, top_k, top_p -- through `slots`
        rows by serve_plan's calls (sampler='philox' only), and yields (position, host float32
        (F_u * lookback,) samples) as requests complete.  Request u's samples are row 0 of the
        one-shot self(slots, 0, cond_u, spk_u, sampler='philox', seed=seed,
        row_offset=stream_id_u, <u's controls>), sample for sample.  If any request carries a
        control, every call passes per-row control arrays (defaults for the other rows).
        self.last_serve: {'calls', 'frames' (per call), 'row_frames'} of the run.
        session=True runs the same plan as the chunks of one GenSession, new requests replacing
        their rows' records by fresh ones: the same yields, without the calls' set-up.
        scores=True yields (position, samples, host float32 (F_u * lookback, 2) scores): row 0 of
        that one-shot call's return_scores result."""
        requests = list(requests)
        slots = int(slots)
        conds = []
        for u, rq in enumerate(requests):
            c = rq['cond']
            c = torch.as_tensor(np.asarray(c) if not torch.is_tensor(c) else c)
            if c.dim() != 2 or c.shape[0] < 1:
                raise ValueError('Generator.serve: request %d: cond must be (frames >= 1, C)' % u)
            conds.append(c.to(torch.float32).cpu())
        plan = serve_plan([c.shape[0] for c in conds], slots, chunk_frames)
        ids = [int(rq.get('stream_id', u)) for u, rq in enumerate(requests)]
        level = (2 if any('top_p' in rq for rq in requests) else
                 1 if any('temperature' in rq or 'top_k' in rq for rq in requests) else 0)
        L = self.model.lookback
        self.last_serve = {'calls': 0, 'frames': [], 'row_frames': 0}
        if not plan:
            return
        C = conds[0].shape[1]
        fresh = self.fresh_state(slots, dtype)
        if session:
            yield from self._serve_session(requests, conds, plan, ids, level, fresh, seed, dtype,
                                           persistent, use_graph, scores)
            return
        state = fresh
        parts, sparts = {}, {}
        for n, rows in plan:
            cond = torch.zeros(slots, n, C)
            spk = torch.zeros(slots, dtype=torch.long)
            sid = torch.zeros(slots, dtype=torch.int64)
            tau, k, p = [1.0] * slots, [0] * slots, [1.0] * slots
            for s, (u, f0, f1, _) in enumerate(rows):
                if u is None:
                    continue
                rq = requests[u]
                cond[s, :f1 - f0] = conds[u][f0:f1]
                spk[s] = int(torch.as_tensor(rq['spk']).reshape(-1)[0])
                sid[s] = ids[u]
                tau[s], k[s], p[s] = (rq.get('temperature', 1.0), rq.get('top_k', 0),
                                      rq.get('top_p', 1.0))
            new = [s for s, row in enumerate(rows) if row[3]]
            if new:
                state = state.replace(new, fresh.rows(new))
            res = self(slots, 0, cond, spk, sampler='philox', seed=seed, dtype=dtype,
                       persistent=persistent, use_graph=use_graph, state=state,
                       return_state=True, stream_ids=sid, temperature=tau, top_k=k,
                       top_p=p, controls_level=level, return_scores=bool(scores))
            out, state = res[0], res[-1]
            self.last_serve['calls'] += 1
            self.last_serve['frames'].append(n)
            self.last_serve['row_frames'] += slots * n
            for s, (u, f0, f1, _) in enumerate(rows):
                if u is None:
                    continue
                parts.setdefault(u, []).append(out[s, :(f1 - f0) * L])
                if scores:
                    sparts.setdefault(u, []).append(res[1][s, :(f1 - f0) * L])
                if f1 == conds[u].shape[0]:
                    if scores:
                        yield u, torch.cat(parts.pop(u)), torch.cat(sparts.pop(u))
                    else:
                        yield u, torch.cat(parts.pop(u))

    def _serve_session(self, requests, conds, plan, ids, level, fresh, seed, dtype, persistent,
                       use_graph, scores=False):
        """serve's calls as the chunks of one session (same plan, same per-row inputs)."""
        slots, C, L = fresh.n_seqs, conds[0].shape[1], self.model.lookback
        parts, sparts = {}, {}
        last_spk = None
        opts = dict(scores=True) if scores else {}
        with self.session(slots, max(n for n, _ in plan), dtype=dtype, level=level, seed=seed,
                          persistent=persistent, use_graph=use_graph, **opts) as sess:
            for n, rows in plan:
                cond = torch.zeros(slots, n, C)
                spk = torch.zeros(slots, dtype=torch.long)
                sid = torch.zeros(slots, dtype=torch.int64)
                tau, k, p = [1.0] * slots, [0] * slots, [1.0] * slots
                for s, (u, f0, f1, _) in enumerate(rows):
                    if u is None:
                        continue
                    rq = requests[u]
                    cond[s, :f1 - f0] = conds[u][f0:f1]
                    spk[s] = int(torch.as_tensor(rq['spk']).reshape(-1)[0])
                    sid[s] = ids[u]
                    tau[s], k[s], p[s] = (rq.get('temperature', 1.0), rq.get('top_k', 0),
                                          rq.get('top_p', 1.0))
                # (a row that has done no step already stands on a fresh record)
                new = [s for s, row in enumerate(rows) if row[3] and int(sess.steps[s]) != 0]
                if new:
                    sess.replace(new, fresh.rows(new))
                ctl = {}
                if level >= 1:
                    ctl.update(temperature=tau, top_k=k)
                if level >= 2:
                    ctl.update(top_p=p)
                same_spk = last_spk is not None and torch.equal(spk, last_spk)
                run = sess.chunk_scored if scores else sess.chunk
                out = run(cond, spk=None if same_spk else spk, stream_ids=sid, **ctl)
                if scores:
                    out, sc = out
                last_spk = spk
                self.last_serve['calls'] += 1
                self.last_serve['frames'].append(n)
                self.last_serve['row_frames'] += slots * n
                for s, (u, f0, f1, _) in enumerate(rows):
                    if u is None:
                        continue
                    parts.setdefault(u, []).append(out[s, :(f1 - f0) * L])
                    if scores:
                        sparts.setdefault(u, []).append(sc[s, :(f1 - f0) * L])
                    if f1 == conds[u].shape[0]:
                        if scores:
                            yield u, torch.cat(parts.pop(u)), torch.cat(sparts.pop(u))
                        else:
                            yield u, torch.cat(parts.pop(u))

    def _stream_session(self, n_seqs, cond, spk, chunk_frames, state, kw):
        """stream's calls as the chunks of one session."""
        kw = dict(kw)
        sampler, noise = kw.pop('sampler', 'torch'), kw.pop('noise', None)
        logp = bool(kw.pop('return_logp', False))
        scores = bool(kw.pop('return_scores', False))
        tau, k, p = kw.pop('temperature', 1.0), kw.pop('top_k', 0), kw.pop('top_p', 1.0)
        ids = kw.pop('stream_ids', None)
        level = max(int(kw.pop('controls_level', 0)),
                    2 if nucleus_control(n_seqs, p) is not None else
                    1 if sampling_controls(n_seqs, tau, k, self.model.q_levels) is not None else 0)
        replay = noise is not None or sampler == 'torch'
        fdim = cond.dim() - 2
        num_cond = cond.shape[fdim]
        L, Q = self.model.lookback, self.model.q_levels
        if state is not None:
            # (the checks of a call that continues `state`)
            if not isinstance(state, GenState):
                raise TypeError('Generator: state must be a GenState')
            if state.n_seqs != n_seqs:
                raise ValueError('Generator: state holds %d rows, the call has %d'
                                 % (state.n_seqs, n_seqs))
            if not replay and ids is None and bool((state.steps != state.steps[0]).any()):
                raise ValueError('Generator: rows at differing step counts %s cannot continue '
                                 'under sampler=\'philox\' (replayed noise can)'
                                 % sorted(set(state.steps.tolist())))
        with self.session(n_seqs, min(chunk_frames, num_cond), level=level, return_logp=logp,
                          replay_noise=replay, scores=scores, **kw) as sess:
            if state is not None:
                sess.replace(list(range(n_seqs)), state)
            ctl = dict(spk=spk, stream_ids=None if replay else ids)
            if level >= 1:
                ctl.update(temperature=tau, top_k=k)
            if level >= 2:
                ctl.update(top_p=p)
            for f0 in range(0, num_cond, chunk_frames):
                f1 = min(num_cond, f0 + chunk_frames)
                q = None
                if replay:
                    q = (noise[f0 * L:f1 * L] if noise is not None else
                         torch.empty((f1 - f0) * L, n_seqs, Q).exponential_(1))
                res = (sess.chunk_scored if scores else sess.chunk)(
                    cond.narrow(fdim, f0, f1 - f0), noise=q, **ctl)
                ctl = {}
                if f1 == num_cond:
                    self.last_state = sess.state()
                yield res

    def stream(self, n_seqs, cond, spk, chunk_frames, state=None, session=False, **kw):
        """Generates chunk_frames conditioning frames per call of __call__, each continuing from
        the state the previous one ended in, and yields every chunk's host float32
        (n_seqs, frames * lookback) block as it completes (with return_logp: (block, logp); with
        return_scores the chunk's (n_seqs, frames * lookback, 2) scores come last: (block,
        scores) or (block, logp, scores)).
        The concatenation equals the single __call__ over all of cond, for either sampler:
        sampler='torch' draws each chunk's noise when the chunk starts -- the CPU generator's
        exponential_ stream does not depend on how it is cut -- so host memory is bounded by
        the chunk; a given `noise` is sliced.  The state after the last chunk is left in
        self.last_state; `state` continues an earlier stream.
        session=True runs the same chunks through one GenSession (no per-call set-up): the same
        yields; self.last_state is then set once, after the last chunk."""
        chunk_frames = int(chunk_frames)
        if chunk_frames < 1:
            raise ValueError('Generator.stream: chunk_frames must be >= 1')
        for name in ('return_state', 'prefix', 'prefix_len'):
            if name in kw:
                raise ValueError('Generator.stream: %s is not a stream argument' % name)
        cond = torch.as_tensor(np.asarray(cond) if not torch.is_tensor(cond) else cond)
        if session:
            yield from self._stream_session(n_seqs, cond, spk, chunk_frames, state, kw)
            return
        fdim = cond.dim() - 2                      # the frame axis of (F, C) or (n_seqs, F, C)
        num_cond = cond.shape[fdim]
        L = self.model.lookback
        noise = kw.pop('noise', None)
        for f0 in range(0, num_cond, chunk_frames):
            f1 = min(num_cond, f0 + chunk_frames)
            res = self(n_seqs, 0, cond.narrow(fdim, f0, f1 - f0), spk, state=state,
                       return_state=True,
                       noise=None if noise is None else noise[f0 * L:f1 * L], **kw)
            state = res[-1]
            self.last_state = state
            yield res[:-1] if len(res) > 2 else res[0]

    def prime(self, prefix, cond, spk, **kw):
        """The GenState after the given audio: a call forced along all of `prefix` ((n_seqs, T)
        indices or a float waveform, T = num_cond * lookback exactly), from which __call__ or
        stream continues with further conditioning frames."""
        prefix = torch.as_tensor(np.asarray(prefix) if not torch.is_tensor(prefix) else prefix)
        if prefix.dim() == 1:
            prefix = prefix.unsqueeze(0)
        cond_t = torch.as_tensor(np.asarray(cond) if not torch.is_tensor(cond) else cond)
        T = cond_t.shape[-2] * self.model.lookback
        if prefix.dim() != 2 or prefix.shape[1] != T:
            raise ValueError('Generator.prime: prefix of shape %s, expected (n_seqs, %d) = '
                             'num_cond * lookback samples' % (tuple(prefix.shape), T))
        kw.setdefault('sampler', 'philox')         # (every step is forced: no noise is needed)
        return self(prefix.shape[0], 0, cond, spk, prefix=prefix, return_state=True, **kw)[-1]


def shard_generate(generator, n_seqs, cond, spk, seed, rank=None, world=None, sampler='philox',
                   seq_len=0, noise_rows=None, **kw):
    """Rank-sharded generation (the reference runs generate.py:241-253 per file on
    one device): rank r generates the contiguous rows [r n / N, (r + 1) n / N) of an n_seqs batch
    with replicated weights and no collective in the loop; the dequantized rows are gathered to
    every rank at the end, and the union equals the single-process output for either sampler:
      * 'philox': the device noise of the GLOBAL rows (row_offset);
      * 'torch' (the reference's multinomial stream, model.py:514-517): every rank draws the
        whole batch's Exp(1) noise from torch's CPU generator exactly as a single process
        would (one (T, n_seqs, Q) draw, so every rank must have been seeded alike) and keeps
        its rows' slice -- host memory T * n_seqs * Q * 4 bytes per rank.  noise_rows: the
        caller's true row count when n_seqs includes padding rows (to a multiple of the world
        size): the draw is then (T, noise_rows, Q), as the unpadded single-process run makes
        it, and the padding rows get unit noise (their output is discarded).
    cond: (num_cond, C) shared or (n_seqs, num_cond, C) per row; spk: int or (n_seqs,).
    temperature / top_k / top_p (Generator's sampling controls): scalars or one value per row of
    the whole batch; per-row values are sliced to the rank's rows like spk.
    seq_len is accepted like Generator's (the reference ignores it, model.py:455).
    Returns the host float32 (n_seqs, num_cond * lookback) batch."""
    import distributed as Dd
    rank = Dd.rank() if rank is None else rank
    world = Dd.world() if world is None else world
    if sampler not in ('philox', 'torch'):
        raise ValueError('shard_generate: unknown sampler %r' % (sampler,))
    rows = Dd.shard_rows(n_seqs, rank, world)
    c = torch.as_tensor(np.asarray(cond) if not torch.is_tensor(cond) else cond)
    num_cond = c.shape[-2]
    if c.dim() == 3:
        c = c[rows]
    s = torch.as_tensor(np.asarray(spk) if not torch.is_tensor(spk) else spk).reshape(-1)
    if s.numel() > 1:
        s = s[rows]
    ctrl = sampling_controls(n_seqs, kw.pop('temperature', 1.0), kw.pop('top_k', 0),
                             generator.model.q_levels)
    if ctrl is not None:
        kw['temperature'], kw['top_k'] = ctrl[0][rows], ctrl[1][rows]
    nucleus = nucleus_control(n_seqs, kw.pop('top_p', 1.0))
    if nucleus is not None:
        kw['top_p'] = nucleus[rows]
    if sampler == 'torch' and kw.get('noise') is None:
        model = generator.model
        nr = n_seqs if noise_rows is None else int(noise_rows)
        if not 0 < nr <= n_seqs:
            raise ValueError('shard_generate: noise_rows %d outside (0, %d]' % (nr, n_seqs))
        full = torch.empty(num_cond * model.lookback, nr, model.q_levels).exponential_(1)
        if nr < n_seqs:
            full = torch.cat([full, full.new_ones((full.shape[0], n_seqs - nr, full.shape[2]))],
                             1)
        kw['noise'] = full[:, rows].contiguous()
        del full
    out = generator(rows.stop - rows.start, seq_len, c, s, sampler=sampler, seed=seed,
                    row_offset=rows.start, **kw)
    return Dd.gather_rows(out, n_seqs)
