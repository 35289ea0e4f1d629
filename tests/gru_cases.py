"""GRU conformance cases: builders, CPU evaluators, references and checkers of the sweep over
the recurrence (csrc/gru.hip, gru_seq.hip, gru_xcd.hip, gru_layer.cpp).

The GRU has transcendentals, so "bit-exact everywhere" (gemm_cases.py) is not available.
Three methods, each where it applies:

  A   forward, exact at saturation.  W_hh in -2..2, b_hh and h0 multiples of 0.5, and the
      input projections +-65536 (gi_n may be 0 where that element's gi_r is -65536): r and z
      are exactly 0 or 1, n exactly -1, 0 or 1, h_t stays in {h0's values, -1, 0, 1} (all
      bf16-exact) and every gh is a sum of multiples of 0.5 below 2^13, exact in fp32 in any
      order.  out, out_lp, the four gate blocks and hprev_lp are compared bit for bit over
      every step: the matmul, the hand-off of h between workgroups, every index and stride.
  B   forward, step-local on random inputs.  Step t is recomputed in float64 from the
      operand the kernel itself consumed (its own out_lp[:, t-1], out[:, t-1] in fp32), so no
      error compounds and a bf16 rounding flip cannot amplify.  The bounds are derived per
      element (_check_fwd_local); the one measured constant is C_FN, the allowance in units
      of 2^-24 for the device's expf / tanhf / divide, measured by method B0 (W_hh = 0).
  C   backward (no transcendentals, contraction off in gru_point.hpp; the inputs need not
      come from a forward run).  Exact for Fr <= 2 on dyadic inputs (every product of the
      point formulas and the dgh . W_hh sum exact in fp32; 'Crne' makes step 1 carry more
      than 8 significant bits, so the round-to-nearest-even of the bf16 hand-off decides),
      step-local with a derived bound carried along the dh chain for longer sequences.

One equivalence before bits are compared: -0.0 is read as +0.0.

Placement.  Every sequence operand is a SeqWindow: (B, Fr, X) elements at
base + b * ld + t * s inside a canary-filled buffer (gemm_cases' canaries); h0, ddir0, bsum
and the weights are gemm_cases Windows.  After a call every output window is fully written,
nothing outside any window changed, and every input buffer is unchanged.

Plain helper module (no fixtures): the CPU test proves the cases, the GPU test runs them.
"""
import dataclasses
import types

import torch

from gemm_cases import Window, _ints, _canary, _esize, _draw, GUARD_ROWS

U = 2.0 ** -24
BIG = 65536.0
NCU = 256                       # CUs of the device the tables are laid out for (MI355X)
# Allowance for the device's expf / tanhf / divide in r, z and n, in units of 2^-24: twice the
# largest error measured against the float64 reference (1.65 on an MI355X, every back end
# within 1.54 .. 1.65: method B0 below), rounded up; the method allows 8 at most.
C_FN = 4.0
DT = {'bf16': torch.bfloat16, 'f32': torch.float32}
BF = torch.bfloat16


# ------------------------------------------------------------------ the sequence window
class SeqWindow:
    """(B, Fr, X) elements at base + b * ld + t * s of a canary-filled 1-D buffer."""

    def __init__(self, dtype, B, Fr, X, ld, s, device, off=0):
        self.dtype, self.B, self.Fr, self.X, self.ld, self.s = dtype, B, Fr, X, ld, s
        al = 16 // _esize(dtype)
        guard = -(-GUARD_ROWS * X // al) * al
        self.base = guard + off
        span = (B - 1) * ld + (Fr - 1) * s + X
        self.buf = torch.empty(self.base + span + guard + al, dtype=dtype, device=device)
        assert self.buf.data_ptr() % 16 == 0
        _ints(self.buf).fill_(_canary(dtype))
        b = torch.arange(B).view(-1, 1, 1) * ld
        t = torch.arange(Fr).view(1, -1, 1) * s
        self.index = (self.base + b + t + torch.arange(X).view(1, 1, -1)).reshape(-1)
        assert (s >= X and ld >= (Fr - 1) * s + X) or (ld >= X and s >= (B - 1) * ld + X) or \
            Fr == 1 or B == 1, 'window rows overlap'
        self.before = None

    def fill(self, values):
        self.buf[self.index.to(self.buf.device)] = values.reshape(-1).to(self.buf)

    def read(self):
        return self.buf[self.index.to(self.buf.device)].view(self.B, self.Fr, self.X).cpu()

    def ptr(self, t=0):
        """Address of element (0, t, 0)."""
        return self.buf.data_ptr() + (self.base + t * self.s) * _esize(self.dtype)

    def snapshot(self):
        self.before = self.buf.clone()

    def unchanged(self):
        return torch.equal(_ints(self.buf), _ints(self.before))

    def written(self):
        """No element of the window still holds the canary."""
        inside = _ints(self.buf)[self.index.to(self.buf.device)]
        return not bool((inside == _canary(self.dtype)).any())

    def all_canary(self):
        return bool((_ints(self.buf) == _canary(self.dtype)).all())

    def outside_ok(self):
        keep = torch.ones(self.buf.numel(), dtype=torch.bool, device=self.buf.device)
        keep[self.index.to(self.buf.device)] = False
        return bool((_ints(self.buf)[keep] == _canary(self.dtype)).all())

    def first_outside(self):
        keep = torch.ones(self.buf.numel(), dtype=torch.bool)
        keep[self.index] = False
        hit = (keep & (_ints(self.buf).cpu() != _canary(self.dtype))).nonzero().view(-1)
        return int(hit[0]), hit.numel()


class FlatWindow(Window):
    """A gemm_cases Window with the SeqWindow's checks (h0, ddir0, bsum, weights, biases)."""

    def ptr(self, t=0):
        return self.view().data_ptr()

    def written(self):
        inside = _ints(self.buf)[self.index.to(self.buf.device)]
        return not bool((inside == _canary(self.dtype)).any())

    def all_canary(self):
        return bool((_ints(self.buf) == _canary(self.dtype)).all())

    def first_outside(self):
        keep = torch.ones(self.buf.numel(), dtype=torch.bool)
        keep[self.index] = False
        hit = (keep & (_ints(self.buf).cpu() != _canary(self.dtype))).nonzero().view(-1)
        return int(hit[0]), hit.numel()

    def read2(self):
        return self.read().cpu()[0]


# ------------------------------------------------------------------ layouts
# Operand classes: gi (3D), o (D: out, out_lp, hprev_lp / hout), g (4D: gates), dy (D),
# d (3D: dgh, dgh_lp, dgi, dgi_lp), x (Din).  Every class gets its own padding and offset;
# the '8' tables keep ldo / so / ldd / sd multiples of 8 and the o / d bases 16-byte aligned,
# which the seq sweeps need (samplernn_hip.h).
PAD = {'gi': 3, 'o': 5, 'g': 7, 'dy': 1, 'd': 9, 'x': 8}
OFF = {'gi': 1, 'o': 3, 'g': 2, 'dy': 1, 'd': 5, 'x': 0}
PAD8 = dict(PAD, o=8, d=16)
OFF8 = dict(OFF, o=8, d=8)
LAYOUTS = ('dense', 'pad', 'tm', 'wide', 'off', 'odd')


def strides(c, op, X):
    """(ld, s, base offset) of an operand class of width X under the case's layout."""
    B, Fr, lay = c.B, c.Fr, c.layout
    al8 = (c.be == 'seq' or c.plan == 'seq') and lay != 'odd'
    pad, off = (PAD8 if al8 else PAD)[op], (OFF8 if al8 else OFF)[op]
    if lay == 'dense':
        return Fr * X, X, 0
    if lay in ('pad', 'odd'):              # every ld padded by a different amount
        return Fr * X + pad, X, 0
    if lay == 'tm':                        # time-major
        return X, B * X, 0
    if lay == 'wide':                      # a step stride beyond the width (sg > 4D, ...)
        return Fr * (X + pad) + pad, X + pad, 0
    if lay == 'off':                       # a base offset
        return Fr * X, X, off
    raise ValueError(lay)


# ------------------------------------------------------------------ the case record
@dataclasses.dataclass(frozen=True)
class Case:
    dir: str                    # 'fwd' / 'bwd'
    be: str                     # 'xcd' 'xcd2' 'seq' 'layer' 'steps'
    method: str                 # 'A' 'B' 'B0' (fwd); 'C' 'Crne' 'Cloc' (bwd)
    dtype: str                  # 'bf16' / 'f32'
    B: int
    D: int
    Fr: int
    layout: str = 'dense'
    plan: str = ''              # layer: the plan the switches leave first
    share: int = 1              # layer: set_device_share for the call
    variant: str = ''           # steps fwd: 'x' (W_ih in the kernel); steps bwd: 'w' 'wt' 'both'
    env: tuple = ()
    expect: str = 'takes'       # 'takes' / 'refuses'

    @property
    def id(self):
        s = '%s-%s-%s-%s-B%dD%dF%d-%s' % (self.dir, self.be + self.plan, self.method, self.dtype,
                                          self.B, self.D, self.Fr, self.layout)
        if self.variant:
            s += '-' + self.variant
        if self.share != 1:
            s += '-share%d' % self.share
        for k, v in self.env:
            s += '-%s=%s' % (k.replace('SRNN_', ''), v)
        if self.expect != 'takes':
            s += '-' + self.expect
        return s

    def envget(self, name, dflt=1):
        return int(dict(self.env).get(name, dflt))


def case(dir, be, method, dtype, B, D, Fr, layout='dense', **kw):
    env = tuple(sorted(kw.pop('env', {}).items()))
    return Case(dir, be, method, dtype, B, D, Fr, layout, env=env, **kw)


# ------------------------------------------------------------------ the dispatchers, restated
def cdiv(a, b):
    return -(-a // b)


def gx_layout(B, D, ncu):
    """gru_xcd.hip's gx_layout: (mt, G, rv, P) or None."""
    if ncu <= 0 or B <= 0 or D % 256 or D > 1024:
        return None
    P = D // 32
    gmax = ncu // P
    if gmax < 1:
        return None
    mt = 1
    while mt < 4 and cdiv(B, 16 * mt) > gmax:
        mt *= 2
    G = cdiv(B, 16 * mt)
    if G > gmax:
        return None
    G = (G + 7) // 8 * 8 if (G + 7) // 8 * 8 <= gmax else G
    rv = cdiv(B, G * mt)
    return (mt, G, rv, P) if rv <= 16 else None


def xcd_route(c, ncu=NCU, fake_strides=None):
    """What gru_try_xcd_fwd / _bwd select for the case: rows per launch and launches, the row
    layout of the first launch, and the kernel selections of the case's direction."""
    B, D, Fr = c.B, c.D, c.Fr
    n = ncu // c.share
    lr = (n // (D // 32)) * 16 * 4 if D % 256 == 0 and D <= 1024 else 0
    if lr <= 0 or c.dtype != 'bf16':
        return None
    rows = min(B, lr)
    L = gx_layout(rows, D, n)
    if L is None:
        return None
    r = dict(lr=lr, chunks=cdiv(B, lr), mt=L[0], G=L[1], rv=L[2], mi={1: 0, 2: 1, 4: 2}[L[0]])
    if c.dir == 'fwd':
        upw = cdiv(D // 32, 8)
        r.update(ui=0 if upw <= 1 else 1 if upw <= 2 else 2,
                 dc=D == 1024 and c.envget('SRNN_GX_DC') != 0)
        return r
    st = fake_strides or {k: strides(c, k, x)[:2] for k, x in
                          (('dy', D), ('g', 4 * D), ('o', D))}
    omax = max(((rows - 1) * st['dy'][0] + (Fr - 1) * st['dy'][1] + D) * 4,
               ((rows - 1) * st['g'][0] + (Fr - 1) * st['g'][1] + 4 * D) * 4,
               ((rows - 1) * st['o'][0] + (Fr - 1) * st['o'][1] + D) * 4, rows * D * 4)
    pk = (D % 64 == 0 and D // 64 <= 16 and (D // 64) % 4 == 0 and Fr < 0x7f80 and
          omax < 0x7fffffff - 64 and c.envget('SRNN_GX_PK') != 0)
    NU = 3 * D // 32
    upw = cdiv(NU, 8)
    ui = 0 if upw <= 3 else 1 if upw <= 6 else 2
    full = NU == (3, 6, 12)[ui] * 8
    lds = 2 * 8 * 2 * 4 * 68 * 4 + 64 + (L[0] * 5 * 512 * 4 if L[0] > 1 else 0)
    r.update(pk=pk, batch=pk and L[0] > 1 and c.envget('SRNN_GX_BATCH') != 0, ui=ui, full=full,
             omax=omax, lds_unpacked=lds)
    return r


def seq_supported(c, ncu=NCU):
    """gru_seq_area != 0."""
    D, B = c.D, c.B
    if c.dtype != 'bf16' or D % 128 or D > 1024 or B <= 0:
        return False
    return (D // 16) * cdiv(B, 32) * c.share <= ncu


def layer_plan(c, ncu=NCU):
    if c.plan == 'xcd' and xcd_route(c, ncu):
        return 'xcd'
    if c.plan in ('xcd', 'seq') and seq_supported(c, ncu):
        return 'seq'
    return 'steps'


def _al16(win, ld, t=0):
    es = _esize(win.dtype)
    return win.ptr(t) % 16 == 0 and (ld * es) % 16 == 0


def steps_route(t):
    """launch_cell's / launch_bwd's conditions for every step of a built steps case: the list of
    booleans 'takes the ring kernel', step by step (the order the calls are made in)."""
    c, w = t.case, t.w
    es = _esize(DT[c.dtype])
    KB = 256 // es
    lp = c.dtype == 'bf16'
    res = []
    if c.dir == 'fwd':
        hw = w['outlp'] if lp else w['out']
        for s in range(c.Fr):
            vec_h = _al16(w['h0lp'], c.D) if s == 0 else _al16(hw, hw.ld, s - 1)
            ring = c.D % KB == 0 and vec_h and _al16(w['whh'], c.D)
            if c.variant == 'x':
                ring = ring and _al16(w['x'], w['x'].ld, s) and _al16(w['wih'], c.D)
            res.append(ring)
        return res
    gw = w['dghlp'] if lp else w['dgh']
    for s in reversed(range(c.Fr)):
        nxt = s + 1 < c.Fr
        vec_wt = 'whht' in w and _al16(w['whht'], 3 * c.D)
        res.append(bool(vec_wt and (3 * c.D) % KB == 0 and (not nxt or _al16(gw, gw.ld, s + 1))))
    return res


# ------------------------------------------------------------------ arithmetic helpers
def bf16r(x):
    """Round to nearest even to bf16, back in float64."""
    return x.float().to(BF).double()


def trunc_bf16(x):
    """A truncating fp32 -> bf16 store (the mutation the sweep must catch)."""
    return ((x.float().contiguous().view(torch.int32) >> 16).to(torch.int16)).view(BF)


def mm32(a, wt, order=0, drop=False):
    """a (M, K) . wt (N, K)^T in fp32, accumulated over k-slices of 32 in ascending (order 0)
    or descending (order 1) order; drop: without the last slice."""
    a, wt = a.float(), wt.float()
    K = a.shape[1]
    cuts = list(range(0, K, 32))
    if drop:
        cuts = cuts[:-1]
    if order:
        cuts = cuts[::-1]
    acc = torch.zeros(a.shape[0], wt.shape[0], dtype=torch.float32)
    for k in cuts:
        sa, sw = a[:, k:k + 32], wt[:, k:k + 32]
        if order:
            sa, sw = sa.flip(1), sw.flip(1)
        acc = acc + sa.contiguous() @ sw.contiguous().t()
    return acc


def bwd_point(dh, r, z, n, ghn, hp):
    """gru_point.hpp, operation by operation, in the tensors' dtype."""
    dn = dh * (1.0 - z)
    dz = dh * (hp - n)
    dan = dn * (1.0 - n * n)
    dr = dan * ghn
    dar = dr * r * (1.0 - r)
    daz = dz * z * (1.0 - z)
    return dar, daz, dan * r, dan, dh * z


# ------------------------------------------------------------------ builders
def _seed(c):
    return (c.B * 1000003 + c.D * 1009 + c.Fr * 17 + len(c.method) * 5 +
            ('fwd', 'bwd').index(c.dir))


def _sw(c, dtype, op, X, device):
    ld, s, off = strides(c, op, X)
    return SeqWindow(dtype, c.B, c.Fr, X, ld, s, device, off)


def _flat(dtype, rows, cols, device, place='tight'):
    return FlatWindow(dtype, rows, cols, place, device)


def _pick(gen, shape, values):
    v = torch.tensor(values, dtype=torch.float64)
    return v[torch.randint(0, len(values), shape, generator=gen)]


def build(c, device='cpu'):
    assert c.dir in ('fwd', 'bwd') and c.layout in LAYOUTS
    return _build_fwd(c, device) if c.dir == 'fwd' else _build_bwd(c, device)


def _build_fwd(c, device):
    assert c.method in ('A', 'B', 'B0')
    gen = torch.Generator().manual_seed(_seed(c))
    B, D, Fr, dt = c.B, c.D, c.Fr, DT[c.dtype]
    lp = c.dtype == 'bf16'
    t = types.SimpleNamespace(case=c, device=device, stats={})
    v = {}
    if c.method == 'A':
        v['whh'] = _draw(gen, (3 * D, D), -2, 2)
        v['bhh'] = _draw(gen, (3 * D,), -2, 2, 0.5)
        v['h0'] = _draw(gen, (B, D), -4, 4, 0.5)
        if c.variant == 'x':
            # gi = x . W_ih^T + b_ih with |x . W_ih^T| <= 2 D and b_ih = +-65536 per unit;
            # n's argument is 0 for the units whose W_ih rows and b_ih are 0 (r = 0 there)
            v['x'] = _draw(gen, (B, Fr, D), -2, 2)
            v['wih'] = _draw(gen, (3 * D, D), -1, 1)
            br = _pick(gen, (D,), (-BIG, BIG))
            bz = _pick(gen, (D,), (-BIG, BIG))
            bn = torch.where(br < 0, _pick(gen, (D,), (-BIG, 0.0, 0.0, BIG)),
                             _pick(gen, (D,), (-BIG, BIG)))
            v['wih'][2 * D:][bn == 0] = 0.0
            v['bih'] = torch.cat([br, bz, bn])
        else:
            gr = _pick(gen, (B, Fr, D), (-BIG, BIG))
            gz = _pick(gen, (B, Fr, D), (-BIG, BIG))
            gn = torch.where(gr < 0, _pick(gen, (B, Fr, D), (-BIG, 0.0, 0.0, BIG)),
                             _pick(gen, (B, Fr, D), (-BIG, BIG)))
            v['gi'] = torch.cat([gr, gz, gn], dim=2)
    else:
        rn = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)
        # B0: W_hh = 0, so gh = b_hh exactly on every back end and the error of r, z and n
        # is the device functions' own (the measurement behind C_FN)
        v['whh'] = (rn(3 * D, D) * (0.0 if c.method == 'B0' else 0.03)).to(dt).double()
        v['bhh'] = (rn(3 * D) * 0.1).float().double()
        v['h0'] = (rn(B, D) * 0.5).float().double()
        if c.variant == 'x':
            v['x'] = (rn(B, Fr, D) * 0.5).to(dt).double()
            v['wih'] = (rn(3 * D, D) * 0.03).to(dt).double()
            v['bih'] = (rn(3 * D) * 0.1).float().double()
        else:
            v['gi'] = (rn(B, Fr, 3 * D) * 0.5).float().double()
    t.values = v
    w = {}
    wplace = 'off1' if c.variant == 'wmis' else 'tight'
    w['whh'] = _flat(dt, 3 * D, D, device, wplace)
    w['whh'].fill(v['whh'])
    w['bhh'] = _flat(torch.float32, 1, 3 * D, device)
    w['bhh'].fill(v['bhh'])
    w['h0'] = _flat(torch.float32, B, D, device)
    w['h0'].fill(v['h0'])
    if c.be in ('seq', 'steps'):        # the caller's `dtype` copy of h0 (fp32: h0 itself)
        w['h0lp'] = _flat(dt, B, D, device)
        w['h0lp'].fill(v['h0'])
    if c.variant == 'x':
        w['x'] = _sw(c, dt, 'x', D, device)
        w['x'].fill(v['x'])
        w['wih'] = _flat(dt, 3 * D, D, device)
        w['wih'].fill(v['wih'])
        w['bih'] = _flat(torch.float32, 1, 3 * D, device)
        w['bih'].fill(v['bih'])
    else:
        w['gi'] = _sw(c, torch.float32, 'gi', 3 * D, device)
        w['gi'].fill(v['gi'])
    t.inputs = sorted(w)
    w['out'] = _sw(c, torch.float32, 'o', D, device)
    if lp:
        w['outlp'] = _sw(c, dt, 'o', D, device)
    w['gates'] = _sw(c, torch.float32, 'g', 4 * D, device)
    if c.be == 'xcd2' or (c.be == 'layer' and c.plan == 'xcd'):
        w['hprev'] = _sw(c, dt, 'o', D, device)
    t.outputs = sorted(k for k in w if k not in t.inputs)
    t.w = w
    for k in t.inputs:
        w[k].snapshot()
    if c.method == 'A':
        _prove_fwd_exact(t)
        t.ref = fwd_chain_ref(t)
    return t


def effective_gi(t):
    """(gi in float64, its error bound): the window's values, or x . W_ih^T + b_ih."""
    c, w = t.case, t.w
    if c.variant != 'x':
        gi = w['gi'].read().double()
        return gi, torch.zeros_like(gi)
    x, wih = w['x'].read().double(), w['wih'].read2().double()
    bih = w['bih'].read2().double().view(-1)
    gi = x @ wih.t() + bih
    return gi, (c.D + 4) * U * (x.abs() @ wih.abs().t() + bih.abs())


def _prove_fwd_exact(t):
    """Method A's preconditions, elementwise in float64."""
    c, v = t.case, t.values
    gi, _ = effective_gi(t)
    D = c.D
    assert bool(((v['whh'] * 1).frac() == 0).all()) and bool(((v['bhh'] * 2).frac() == 0).all())
    # h stays within +-2 (h0's range, or -1 / 0 / 1), multiples of 0.5: every partial sum of
    # gh is a multiple of 0.5 below 2 * sum |w| + |b| < 2^13 -- 14 bits
    assert float((2 * v['whh'].abs().sum(1) + v['bhh'].abs()).max()) < 2.0 ** 13
    assert bool(((gi[..., :2 * D].abs() - BIG).abs() <= 2 * D).all())
    gn, gr = gi[..., 2 * D:], gi[..., :D]
    assert bool((((gn.abs() - BIG).abs() <= 2 * D) | ((gn == 0) & (gr < 0))).all())


def fwd_chain_ref(t):
    """The float64 recurrence on its own chain (Method A: every value exact)."""
    c, w = t.case, t.w
    lp = c.dtype == 'bf16'
    W, b = w['whh'].read2().double(), w['bhh'].read2().double().view(-1)
    gi, _ = effective_gi(t)
    h = w['h0'].read2().double()
    D = c.D
    out, gates, hprev = [], [], []
    for s in range(c.Fr):
        hm = bf16r(h) if lp else h
        hprev.append(hm)
        gh = hm @ W.t() + b
        a = gi[:, s] + torch.cat([gh[:, :2 * D], torch.zeros_like(gh[:, 2 * D:])], 1)
        r, z = torch.sigmoid(a[:, :D]), torch.sigmoid(a[:, D:2 * D])
        n = torch.tanh(gi[:, s, 2 * D:] + gh[:, 2 * D:] * r)
        h = (h - n) * z + n
        out.append(h)
        gates.append(torch.cat([r, z, n, gh[:, 2 * D:]], 1))
    ref = dict(out=torch.stack(out, 1), gates=torch.stack(gates, 1))
    ref['outlp'] = bf16r(ref['out'])
    ref['hprev'] = torch.stack(hprev, 1)
    return ref


def _build_bwd(c, device):
    assert c.method in ('C', 'Crne', 'Cloc')
    gen = torch.Generator().manual_seed(_seed(c))
    B, D, Fr, dt = c.B, c.D, c.Fr, DT[c.dtype]
    lp = c.dtype == 'bf16'
    t = types.SimpleNamespace(case=c, device=device, stats={})
    v = {}
    if c.method == 'Cloc':
        rn = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)
        v['whh'] = (rn(3 * D, D) * 0.03).to(dt).double()
        v['gates'] = torch.cat([torch.sigmoid(rn(B, Fr, 2 * D)), torch.tanh(rn(B, Fr, D)),
                                rn(B, Fr, D) * 0.5], 2).float().double()
        v['hout'] = (rn(B, Fr, D) * 0.5).float().double()
        v['h0'] = (rn(B, D) * 0.5).float().double()
        v['dy'] = (rn(B, Fr, D) * 0.1).float().double()
    else:
        assert Fr in (1, 2)
        rne = c.method == 'Crne'
        v['whh'] = _draw(gen, (3 * D, D), -2, 2)
        sh = (B, 1, D)
        # the last step (t = Fr - 1): its dgh feeds the matmul
        r1 = _pick(gen, sh, (0.25, 0.75) if rne else (0, 0.25, 0.5, 0.75, 1))
        z1 = _pick(gen, sh, (0, 0.5, 1) if rne else (0, 0.25, 0.5, 0.75, 1))
        n1 = _pick(gen, sh, (-1, 0, 0, 1) if rne else (-1, -0.5, 0, 0.5, 1))
        g1 = _pick(gen, sh, (-2, -1, 0, 1, 2) if rne else (-2, -1, 0, 0.5, 1, 2))
        hp1 = _draw(gen, (B, D), -4, 4, 0.5)
        dy1 = _draw(gen, sh, -2, 2)
        if rne:
            dy1 = dy1 * (2 * torch.randint(0, 128, sh, generator=gen).double() + 1)
        last = torch.cat([r1, z1, n1, g1], 2)
        if Fr == 1:
            v['gates'], v['dy'], v['h0'] = last, dy1, hp1
            v['hout'] = _draw(gen, (B, 1, D), -4, 4, 0.5)          # (h_0: not read)
        else:
            r0, z0 = _pick(gen, sh, (0, 0.5, 1)), _pick(gen, sh, (0, 0.5, 1))
            n0 = _pick(gen, sh, (-1, 0, 1))
            g0 = _draw(gen, sh, -2, 2)
            v['gates'] = torch.cat([torch.cat([r0, z0, n0, g0], 2), last], 1)
            v['h0'] = n0[:, 0] + _pick(gen, (B, D), (0, 0.5, -0.5, 1, -1, 2, -2))
            v['dy'] = torch.cat([_draw(gen, sh, -4, 4), dy1], 1)
            # h_0 is step 1's h_prev; h_1 is not read
            v['hout'] = torch.cat([hp1.view(sh), _draw(gen, sh, -4, 4, 0.5)], 1)
    t.values = v
    w = {}
    # W_hh (3D, D): the layer entry and the steps ('w', 'both'); W_hh^T (D, 3D): everyone but
    # the steps' 'w'.  'wmis': W_hh^T one element past a 16-byte boundary
    if c.be == 'layer' or (c.be == 'steps' and c.variant != 'wt'):
        w['whh'] = _flat(dt, 3 * D, D, device)
        w['whh'].fill(v['whh'])
    if not (c.be == 'steps' and c.variant == 'w'):
        w['whht'] = _flat(dt, D, 3 * D, device, 'off1' if c.variant == 'wmis' else 'tight')
        w['whht'].fill(v['whh'].t())
    w['dy'] = _sw(c, torch.float32, 'dy', D, device)
    w['dy'].fill(v['dy'])
    w['gates'] = _sw(c, torch.float32, 'g', 4 * D, device)
    w['gates'].fill(v['gates'])
    w['hout'] = _sw(c, torch.float32, 'o', D, device)
    w['hout'].fill(v['hout'])
    w['h0'] = _flat(torch.float32, B, D, device)
    w['h0'].fill(v['h0'])
    t.inputs = sorted(w)
    xcd_all = c.be == 'xcd2' or (c.be == 'layer' and c.plan == 'xcd')
    w['dgh'] = _sw(c, torch.float32, 'd', 3 * D, device)
    w['dgi'] = _sw(c, torch.float32, 'd', 3 * D, device)
    if lp:
        w['dghlp'] = _sw(c, dt, 'd', 3 * D, device)
    if xcd_all:
        w['dgilp'] = _sw(c, dt, 'd', 3 * D, device)
        w['bsum'] = _flat(torch.float32, B, 4 * D, device)
    w['ddir0'] = _flat(torch.float32, B, D, device)
    t.outputs = sorted(k for k in w if k not in t.inputs)
    t.w = w
    for k in t.inputs:
        w[k].snapshot()
    if c.method != 'Cloc':
        t.ref = bwd_chain_ref(t)
        _prove_bwd_exact(t)
    return t


def _weights_t(t):
    """W_hh^T (D, 3D) in float64 from whichever form the case holds."""
    w = t.w
    return w['whht'].read2().double() if 'whht' in w else w['whh'].read2().double().t()


def bwd_chain_ref(t):
    """The float64 reverse sweep on its own chain; the matmul operand is the bf16 rounding
    (to nearest even) of its own dgh (bf16) or dgh itself (fp32)."""
    c, w = t.case, t.w
    lp = c.dtype == 'bf16'
    D, Fr = c.D, c.Fr
    Wt = _weights_t(t)
    gt, hout = w['gates'].read().double(), w['hout'].read().double()
    h0, dy = w['h0'].read2().double(), w['dy'].read().double()
    dgh, dgi = [None] * Fr, [None] * Fr
    ddir = None
    bsum = torch.zeros(c.B, 4 * D, dtype=torch.float64)
    ref = {}
    for s in reversed(range(Fr)):
        dh = dy[:, s]
        if s + 1 < Fr:
            g = bf16r(dgh[s + 1]) if lp else dgh[s + 1]
            dh = dh + ddir + g @ Wt.t()
        ref['dh%d' % s] = dh
        r, z, n, ghn = (gt[:, s, k * D:(k + 1) * D] for k in range(4))
        hp = hout[:, s - 1] if s else h0
        dar, daz, dghn, dan, ddir = bwd_point(dh, r, z, n, ghn, hp)
        dgh[s] = torch.cat([dar, daz, dghn], 1)
        dgi[s] = torch.cat([dar, daz, dan], 1)
        # two terms at most: whatever the order, one rounding of the exact sum
        bsum = bsum + torch.cat([dar, daz, dghn, dan], 1)
    ref.update(dgh=torch.stack(dgh, 1), dgi=torch.stack(dgi, 1), ddir0=ddir,
               bsum=bsum.float().double())
    ref['dghlp'], ref['dgilp'] = bf16r(ref['dgh']), bf16r(ref['dgi'])
    return ref


def _prove_bwd_exact(t):
    """Method C's preconditions: the hand-off operand's values are multiples of q and
    sum |g w| / q < 2^24, so every partial sum of dgh . W_hh is exact in fp32 in any order,
    and every output is an fp32 number."""
    c, ref = t.case, t.ref
    for k in ('dgh', 'dgi', 'ddir0', 'dh0'):
        assert torch.equal(ref[k].float().double(), ref[k]), '%s: %s is not fp32-exact' % (c.id, k)
    if c.Fr < 2:
        return
    q = 2.0 ** -5 if c.method == 'Crne' else 2.0 ** -9
    g = (bf16r(ref['dgh'][:, 1]) if c.dtype == 'bf16' else ref['dgh'][:, 1])
    z1 = t.w['gates'].read().double()[:, 1, c.D:2 * c.D]
    dy0, ddir1 = t.w['dy'].read().double()[:, 0], ref['dh1'] * z1
    for x in (g, dy0, ddir1):
        assert bool(((x / q).frac() == 0).all()), '%s: step 0 operand not on the grid' % c.id
    bound = (g.abs() @ _weights_t(t).abs().t() + dy0.abs() + ddir1.abs()) / q
    assert float(bound.max()) < 2.0 ** 24, '%s: the hand-off sum is not exact' % c.id
    if c.method == 'C' and c.dtype == 'bf16':
        assert torch.equal(bf16r(ref['dgh'][:, 1]), ref['dgh'][:, 1]), 'step 1 not bf16-exact'


# ------------------------------------------------------------------ CPU evaluators (fp32)
def _store(t, name, values, mut):
    w = t.w[name]
    vals = values
    if mut == 'row_dup' and t.case.B > 1:
        vals = values.clone()
        vals[-1] = vals[-2]
    w.fill(vals)


def evaluate_fwd(t, order=0, mut=None):
    """What a correct fp32 kernel leaves behind (k-slices summed in `order`), written into the
    output windows; `mut` names one defect to build in."""
    c, w = t.case, t.w
    lp = c.dtype == 'bf16'
    D, Fr, dt = c.D, c.Fr, DT[c.dtype]
    W, b = w['whh'].read2().float(), w['bhh'].read2().float().view(-1)
    if c.variant == 'x':
        x, wih = w['x'].read(), w['wih'].read2()
        bih = w['bih'].read2().float().view(-1)
        gi = torch.stack([mm32(x[:, s], wih, order) + bih for s in range(Fr)], 1)
    else:
        gi = w['gi'].read().float()
    h = w['h0'].read2().float()
    ops = [h.to(dt).float()]                     # the matmul operands, step by step
    out, outlp, gates, hprev = [], [], [], []
    for s in range(Fr):
        hm = ops[-1]
        if mut == 'h0_at_1' and s == 1:
            hm = ops[0]
        if mut == 'stale_h' and s >= 2:
            hm = hm.clone()
            hm[:, 3] = ops[-2][:, 3]
        gh = mm32(hm, W, order, drop=mut == 'drop_k') + b
        r = 1.0 / (1.0 + torch.exp(-(gh[:, :D] + gi[:, s, :D])))
        z = 1.0 / (1.0 + torch.exp(-(gh[:, D:2 * D] + gi[:, s, D:2 * D])))
        ghn = gh[:, 2 * D:]
        n = torch.tanh(gi[:, s, 2 * D:] + ghn * r)
        h = (h - n) * z + n
        hl = trunc_bf16(h) if mut == 'trunc' else h.to(dt)
        out.append(h)
        outlp.append(hl)
        hprev.append(ops[-1].to(dt))
        ops.append(hl.float())
        gates.append(torch.cat([z, r, n, ghn] if mut == 'swap_rz' else [r, z, n, ghn], 1))
    _store(t, 'out', torch.stack(out, 1), mut)
    _store(t, 'gates', torch.stack(gates, 1), mut)
    if lp:
        _store(t, 'outlp', torch.stack(outlp, 1), mut)
    if 'hprev' in w:
        _store(t, 'hprev', torch.stack(hprev, 1), mut)
    if mut == 'canary':
        x = w['out']
        keep = torch.ones(x.buf.numel(), dtype=torch.bool)
        keep[x.index] = False
        gap = keep.nonzero().view(-1)
        x.buf[int(gap[gap > x.base][0])] = 0.5      # the first gap element after the base


def evaluate_bwd(t, order=0, mut=None):
    c, w = t.case, t.w
    lp = c.dtype == 'bf16'
    D, Fr, dt = c.D, c.Fr, DT[c.dtype]
    Wt = _weights_t(t).float()
    gt, hout = w['gates'].read().float(), w['hout'].read().float()
    h0, dy = w['h0'].read2().float(), w['dy'].read().float()
    dgh, dgi, glp, gilp = [None] * Fr, [None] * Fr, [None] * Fr, [None] * Fr
    ddirs = [None] * Fr
    bsum = torch.zeros(c.B, 4 * D)
    for s in reversed(range(Fr)):
        dh = dy[:, s]
        if s + 1 < Fr:
            dh = mm32(glp[s + 1].float(), Wt, order, drop=mut == 'drop_k') + dh
            dh = dh + ddirs[s + 1]
        if mut == 'dh_rel' and s == 0:
            dh = dh.clone()
            k = int((dh[0].abs() * gt[0, 0, D:2 * D]).argmax())    # (z > 0: dh reaches ddir0)
            dh[0, k] = dh[0, k] * (1.0 + 1e-4)
        r, z, n, ghn = (gt[:, s, k * D:(k + 1) * D] for k in range(4))
        hp = hout[:, s - 1] if s else h0
        dar, daz, dghn, dan, ddirs[s] = bwd_point(dh, r, z, n, ghn, hp)
        dgh[s], dgi[s] = torch.cat([dar, daz, dghn], 1), torch.cat([dar, daz, dan], 1)
        glp[s] = (trunc_bf16(dgh[s]) if mut == 'trunc' else dgh[s].to(dt)) if lp else dgh[s]
        gilp[s] = dgi[s].to(BF)
        bsum = bsum + torch.cat([dar, daz, dghn, dan], 1)
    _store(t, 'dgh', torch.stack(dgh, 1), mut)
    _store(t, 'dgi', torch.stack(dgi, 1), mut)
    if lp:
        _store(t, 'dghlp', torch.stack(glp, 1), mut)
    if 'dgilp' in w:
        _store(t, 'dgilp', torch.stack(gilp, 1), mut)
        _store(t, 'bsum', bsum, mut)
    _store(t, 'ddir0', ddirs[1] if mut == 'ddir0_from_1' and Fr > 1 else ddirs[0], mut)
    if mut == 'canary':
        x = w['dgh']
        keep = torch.ones(x.buf.numel(), dtype=torch.bool)
        keep[x.index] = False
        gap = keep.nonzero().view(-1)
        x.buf[int(gap[gap > x.base][0])] = 0.5


def evaluate(t, order=0, mut=None):
    (evaluate_fwd if t.case.dir == 'fwd' else evaluate_bwd)(t, order, mut)


# ------------------------------------------------------------------ checkers
def _where(t, name, flat_index):
    """Element name of a flat index into a (B, Fr, X) or (B, X) block."""
    c = t.case
    X = {'gates': 4 * c.D, 'dgh': 3 * c.D, 'dgi': 3 * c.D, 'dghlp': 3 * c.D, 'dgilp': 3 * c.D,
         'bsum': 4 * c.D}.get(name, c.D)
    if name in ('ddir0', 'bsum'):
        b, x = divmod(flat_index, X)
        return 'row %d, block %d, unit %d' % (b, x // c.D, x % c.D)
    b, rest = divmod(flat_index, c.Fr * X)
    s, x = divmod(rest, X)
    return 'row %d, step %d, block %d, unit %d' % (b, s, x // c.D, x % c.D)


def _bits(x, dtype):
    return _ints((x.to(torch.float32) + 0.0).to(dtype) + 0.0)


def _exact(t, bad, name, got, want, dtype):
    """got (as read) against want (float64), bit for bit in `dtype`."""
    g, wv = _bits(got, dtype), _bits(want, dtype)
    diff = (g != wv).reshape(-1)
    if bool(diff.any()):
        i = int(diff.nonzero()[0])
        bad.append('%s: %d of %d elements differ, first at (%s): got %r, want %r' % (
            name, int(diff.sum()), diff.numel(), _where(t, name, i),
            float(got.reshape(-1)[i]), float(want.reshape(-1)[i])))


def _within(t, bad, name, got, want, bound):
    """|got - want| <= bound elementwise; NaN fails."""
    err = (got.double() - want).abs()
    over = (~(err <= bound)).reshape(-1)
    if bool(over.any()):
        i = int(over.nonzero()[0])
        bad.append('%s: %d of %d elements out of bound, first at (%s): got %r, want %r, '
                   'bound %.3g' % (name, int(over.sum()), over.numel(), _where(t, name, i),
                                   float(got.reshape(-1)[i]), float(want.reshape(-1)[i]),
                                   float(bound.reshape(-1)[i])))


def _read(t, name):
    x = t.w[name]
    return x.read() if isinstance(x, SeqWindow) else x.read2()


def _check_windows(t, bad):
    for k in t.outputs:
        x = t.w[k]
        if not x.written():
            inside = _ints(x.buf)[x.index.to(x.buf.device)].cpu()
            i = int((inside == _canary(x.dtype)).nonzero()[0])
            bad.append('%s: %d elements of the window were not written, first at (%s)' % (
                k, int((inside == _canary(x.dtype)).sum()), _where(t, k, i)))
        if not x.outside_ok():
            e, n = x.first_outside()
            bad.append('outside the %s window: %d canary elements overwritten, first at buffer '
                       'element %d (window base %d, ld %d, s %d)' % (
                           k, n, e, getattr(x, 'base', getattr(x, 'front', 0)), x.ld,
                           getattr(x, 's', 0)))
    for k in t.inputs:
        if not t.w[k].unchanged():
            bad.append('input buffer %s was written' % k)


def _check_fwd_exact(t, bad):
    c, ref = t.case, t.ref
    _exact(t, bad, 'out', _read(t, 'out'), ref['out'], torch.float32)
    _exact(t, bad, 'gates', _read(t, 'gates'), ref['gates'], torch.float32)
    if 'outlp' in t.w:
        _exact(t, bad, 'outlp', _read(t, 'outlp'), ref['outlp'], BF)
    if 'hprev' in t.w:
        _exact(t, bad, 'hprev', _read(t, 'hprev'), ref['hprev'], BF)


def _check_fwd_local(t, bad):
    """Method B.  Step t in float64 from the operand the kernel consumed, each value with its
    bound beside it."""
    c, w = t.case, t.w
    lp = c.dtype == 'bf16'
    D, Fr = c.D, c.Fr
    W, b = w['whh'].read2().double(), w['bhh'].read2().double().view(-1)
    gi, egi = effective_gi(t)
    h0 = w['h0'].read2().double()
    out, gk = _read(t, 'out'), _read(t, 'gates')
    outlp = _read(t, 'outlp') if lp else out
    want, bound = [], []
    hwant, hbound = [], []
    for s in range(Fr):
        hm = (outlp[:, s - 1].double() if s else (bf16r(h0) if lp else h0))
        hp = out[:, s - 1].double() if s else h0
        gh = hm @ W.t() + b
        egh = (D + 4) * U * (hm.abs() @ W.abs().t() + b.abs())
        a = gi[:, s, :2 * D] + gh[:, :2 * D]
        rz = torch.sigmoid(a)
        erz = 0.25 * (egh[:, :2 * D] + egi[:, s, :2 * D] +
                      U * (gh[:, :2 * D].abs() + gi[:, s, :2 * D].abs())) + C_FN * U
        r, er = rz[:, :D], erz[:, :D]
        ghn, eghn = gh[:, 2 * D:], egh[:, 2 * D:]
        gin = gi[:, s, 2 * D:]
        n = torch.tanh(gin + ghn * r)
        en = (eghn * r + ghn.abs() * er + egi[:, s, 2 * D:] +
              U * (2 * (ghn * r).abs() + gin.abs())) + C_FN * U
        want.append(torch.cat([rz, n, ghn], 1))
        bound.append(torch.cat([erz, en, eghn], 1))
        # h_t from the kernel's own stored r, z, n and fp32 h_{t-1}
        zk, nk = gk[:, s, D:2 * D].double(), gk[:, s, 2 * D:3 * D].double()
        hwant.append((hp - nk) * zk + nk)
        hbound.append(4 * U * (hp.abs() + 2 * nk.abs()))
    want, bound = torch.stack(want, 1), torch.stack(bound, 1)
    _within(t, bad, 'gates', gk, want, bound)
    # the function allowance actually used, in units of 2^-24 (the measurement behind C_FN)
    fn = ((gk.double() - want).abs() / U)
    t.stats['fn_err_u'] = float(fn.view(c.B, Fr, 4, D)[:, :, :3].max())
    _within(t, bad, 'out', out, torch.stack(hwant, 1), torch.stack(hbound, 1))
    if lp:
        _exact(t, bad, 'outlp', outlp, out.double(), BF)                 # == bf16_rne(out)
    if 'hprev' in w:
        first = bf16r(h0).view(c.B, 1, D)
        _exact(t, bad, 'hprev', _read(t, 'hprev'),
               torch.cat([first, outlp[:, :-1].double()], 1), BF)


def _check_bwd_exact(t, bad):
    ref = t.ref
    for k in ('dgh', 'dgi', 'ddir0', 'bsum'):
        if k in t.w:
            _exact(t, bad, k, _read(t, k), ref[k], torch.float32)
    for k in ('dghlp', 'dgilp'):
        if k in t.w:
            _exact(t, bad, k, _read(t, k), ref[k], BF)


def _check_bwd_local(t, bad):
    """Method C, step-local.  The float64 reference carries its own dh chain; the matmul operand
    of step t is the kernel's own dgh_lp[:, t+1] (dgh in fp32).  err(dh_t) = err(dh_{t+1}) z_{t+1}
    + (3D + 8) 2^-24 (|dy| + |ddir| + sum_k |g_k w_k|), pushed through every operation of the
    point formulas with that operation's rounding.  Nothing in the bound is measured."""
    c, w = t.case, t.w
    lp = c.dtype == 'bf16'
    D, Fr = c.D, c.Fr
    Wt = _weights_t(t)
    gt, hout = w['gates'].read().double(), w['hout'].read().double()
    h0, dy = w['h0'].read2().double(), w['dy'].read().double()
    kdgh, kdgi = _read(t, 'dgh'), _read(t, 'dgi')
    kop = _read(t, 'dghlp') if lp else kdgh
    R = 1.001 * U                 # one rounding (second-order terms in the margin)
    dgh, dgi, egh, egi = [None] * Fr, [None] * Fr, [None] * Fr, [None] * Fr
    ddir = eddir = None
    bs = torch.zeros(c.B, 4 * D, dtype=torch.float64)
    ebs, abs_ = torch.zeros_like(bs), torch.zeros_like(bs)
    for s in reversed(range(Fr)):
        dh, edh = dy[:, s], torch.zeros(c.B, D, dtype=torch.float64)
        if s + 1 < Fr:
            g = kop[:, s + 1].double()
            dh = dh + ddir + g @ Wt.t()
            edh = eddir + (3 * D + 8) * U * (dy[:, s].abs() + ddir.abs() + g.abs() @ Wt.abs().t())
        r, z, n, ghn = (gt[:, s, k * D:(k + 1) * D] for k in range(4))
        hp = hout[:, s - 1] if s else h0
        # every operation of gru_point.hpp with its own rounding (R per result); the
        # differences 1 - z, 1 - r and h_prev - n of fp32 inputs round once, and 1 - n * n
        # carries the rounding of n * n as an absolute error, which matters where |n| is near 1
        q1, q2, q3, q4 = 1 - z, hp - n, 1 - n * n, 1 - r
        a1, a2, a3, a4 = R * q1.abs(), R * q2.abs(), R * (n * n + q3.abs()), R * q4.abs()
        dn, dz = dh * q1, dh * q2
        edn = edh * q1.abs() + dh.abs() * a1 + R * dn.abs()
        edz = edh * q2.abs() + dh.abs() * a2 + R * dz.abs()
        dan = dn * q3
        edan = edn * q3.abs() + dn.abs() * a3 + R * dan.abs()
        dr = dan * ghn
        edr = edan * ghn.abs() + R * dr.abs()
        t1, t2 = dr * r, dz * z
        et1, et2 = edr * r + R * t1.abs(), edz * z + R * t2.abs()
        dar, daz = t1 * q4, t2 * q1
        edar = et1 * q4.abs() + t1.abs() * a4 + R * dar.abs()
        edaz = et2 * q1.abs() + t2.abs() * a1 + R * daz.abs()
        dghn = dan * r
        edghn = edan * r + R * dghn.abs()
        ddir, eddir = dh * z, edh * z + R * (dh * z).abs()
        dgh[s], egh[s] = torch.cat([dar, daz, dghn], 1), torch.cat([edar, edaz, edghn], 1)
        dgi[s], egi[s] = torch.cat([dar, daz, dan], 1), torch.cat([edar, edaz, edan], 1)
        term = torch.cat([dar, daz, dghn, dan], 1)
        bs, abs_ = bs + term, abs_ + term.abs()
        ebs = ebs + torch.cat([edar, edaz, edghn, edan], 1)
    _within(t, bad, 'dgh', kdgh, torch.stack(dgh, 1), torch.stack(egh, 1))
    _within(t, bad, 'dgi', kdgi, torch.stack(dgi, 1), torch.stack(egi, 1))
    _within(t, bad, 'ddir0', _read(t, 'ddir0'), ddir, eddir)
    if lp:
        _exact(t, bad, 'dghlp', kop, kdgh.double(), BF)                  # == bf16_rne(dgh)
    if 'dgilp' in w:
        _exact(t, bad, 'dgilp', _read(t, 'dgilp'), kdgi.double(), BF)
        _within(t, bad, 'bsum', _read(t, 'bsum'), bs, ebs + (Fr + 2) * U * abs_)


def check(t):
    """None when the built case's buffers hold a conforming result, else the report."""
    bad = []
    _check_windows(t, bad)
    {'A': _check_fwd_exact, 'B': _check_fwd_local, 'B0': _check_fwd_local, 'C': _check_bwd_exact,
     'Crne': _check_bwd_exact, 'Cloc': _check_bwd_local}[t.case.method](t, bad)
    return '%s: %s' % (t.case.id, '; '.join(bad)) if bad else None


def untouched(t):
    """Every output buffer is canary throughout (a refusal wrote nothing)."""
    return all(t.w[k].all_canary() for k in t.outputs)


# ------------------------------------------------------------------ running a case on the GPU
def _work(nbytes, device):
    return torch.full((max(nbytes, 16),), 7, device=device, dtype=torch.uint8)


def _p(t, name, step=0):
    return t.w[name].ptr(step) if name in t.w else None


def plan_env(c):
    """The environment of a case: its own switches, and for the layer entry the two plan
    switches that leave `plan` first (test_gpu_gru_layer.py's `switches`)."""
    env = {'SRNN_GRU_XCD': None, 'SRNN_GRU_SEQ': None}
    if c.be == 'layer':
        if c.plan in ('seq', 'steps'):
            env['SRNN_GRU_XCD'] = '0'
        if c.plan == 'steps':
            env['SRNN_GRU_SEQ'] = '0'
    env.update(dict(c.env))
    return env


def run(hip, t):
    """Launch the built case through its entry point; returns the XCD work buffers (their
    first word is the sweep's error word)."""
    return (_run_fwd if t.case.dir == 'fwd' else _run_bwd)(hip, t)


def _run_fwd(hip, t):
    c, w = t.case, t.w
    B, D, Fr, dc = c.B, c.D, c.Fr, hip.dcode(DT[c.dtype])
    lp = c.dtype == 'bf16'
    call, st = hip.lib().call, hip.stream()
    gi, o, g = w.get('gi'), w['out'], w['gates']
    p = lambda name, s=0: _p(t, name, s)
    works = []
    if c.be in ('xcd', 'xcd2'):
        nb = hip.gru_xcd_work_bytes(DT[c.dtype], B, D)
        assert nb, 'the XCD forward does not take this shape here'
        wk = _work(nb, t.device)
        works.append(wk)
        args = (dc, B, D, Fr, p('gi'), gi.ld, gi.s, p('h0'), p('whh'), p('bhh'), p('out'),
                p('outlp'), o.ld, o.s, p('gates'), g.ld, g.s)
        if c.be == 'xcd':
            call('srnn_gru_xcd_fwd', *args, wk.data_ptr(), nb, st)
        else:
            call('srnn_gru_xcd_fwd2', *args, p('hprev'), wk.data_ptr(), nb, st)
    elif c.be == 'seq':
        assert hip.gru_seq_supported(DT[c.dtype], B, D)
        nb = (64 * ((B + 31) // 32) + 1) * 4
        wk = _work(nb, t.device)
        call('srnn_gru_seq_fwd', dc, B, D, Fr, p('gi'), gi.ld, gi.s, p('h0'), p('h0lp'), p('whh'),
             p('bhh'), p('out'), p('outlp'), o.ld, o.s, p('gates'), g.ld, g.s, wk.data_ptr(), nb,
             st)
    elif c.be == 'layer':
        be, nf, _ = hip.gru_layer_plan(DT[c.dtype], B, D)
        assert be == c.plan, 'the plan is %s, the case wants %s' % (be, c.plan)
        wk = _work(nf, t.device)
        if be == 'xcd':
            works.append(wk)
        call('srnn_gru_layer_fwd', dc, B, D, Fr, p('gi'), gi.ld, gi.s, p('h0'), p('whh'), p('bhh'),
             p('out'), p('outlp'), o.ld, o.s, p('gates'), g.ld, g.s, p('hprev'),
             wk.data_ptr() if nf else None, nf, st)
    else:
        hl = w['outlp'] if lp else w['out']
        for s in range(Fr):
            h, ldh = (p('h0lp'), D) if s == 0 else (hl.ptr(s - 1), hl.ld)
            hf, ldhf = (p('h0'), D) if s == 0 else (o.ptr(s - 1), o.ld)
            if c.variant == 'x':
                x = w['x']
                call('srnn_gru_cell', dc, B, D, D, x.ptr(s), x.ld, p('wih'), p('bih'), None, 0, h,
                     ldh, hf, ldhf, p('whh'), p('bhh'), o.ptr(s), o.ld, p('outlp', s), o.ld,
                     g.ptr(s), g.ld, st)
            else:
                call('srnn_gru_cell', dc, B, D, D, None, 0, None, None, gi.ptr(s), gi.ld, h, ldh,
                     hf, ldhf, p('whh'), p('bhh'), o.ptr(s), o.ld, p('outlp', s), o.ld, g.ptr(s),
                     g.ld, st)
    return works


def _run_bwd(hip, t):
    c, w = t.case, t.w
    B, D, Fr, dc = c.B, c.D, c.Fr, hip.dcode(DT[c.dtype])
    lp = c.dtype == 'bf16'
    call, st = hip.lib().call, hip.stream()
    dy, g, o, d = w['dy'], w['gates'], w['hout'], w['dgh']
    p = lambda name, s=0: _p(t, name, s)
    works = []
    if c.be in ('xcd', 'xcd2'):
        nb = hip.gru_xcd_bwd_work_bytes(DT[c.dtype], B, D)
        assert nb, 'the XCD backward does not take this shape here'
        wk = _work(nb, t.device)
        works.append(wk)
        head = (dc, B, D, Fr, p('dy'), dy.ld, dy.s, p('gates'), g.ld, g.s, p('hout'), o.ld, o.s,
                p('h0'), p('whht'), p('dgh'), p('dghlp'), p('dgi'))
        if c.be == 'xcd':
            call('srnn_gru_xcd_bwd', *head, d.ld, d.s, p('ddir0'), wk.data_ptr(), nb, st)
        else:
            call('srnn_gru_xcd_bwd2', *head, p('dgilp'), p('bsum'), d.ld, d.s, p('ddir0'),
                 wk.data_ptr(), nb, st)
    elif c.be == 'seq':
        assert hip.gru_seq_supported(DT[c.dtype], B, D)
        nb = (64 * ((B + 31) // 32) + 1) * 4
        wk = _work(nb, t.device)
        call('srnn_gru_seq_bwd', dc, B, D, Fr, p('dy'), dy.ld, dy.s, p('gates'), g.ld, g.s,
             p('hout'), o.ld, o.s, p('h0'), p('whht'), p('dgh'), p('dghlp'), p('dgi'), d.ld, d.s,
             p('ddir0'), wk.data_ptr(), nb, st)
    elif c.be == 'layer':
        be, _, nb = hip.gru_layer_plan(DT[c.dtype], B, D)
        assert be == c.plan, 'the plan is %s, the case wants %s' % (be, c.plan)
        wk = _work(nb, t.device)
        if be == 'xcd':
            works.append(wk)
        call('srnn_gru_layer_bwd', dc, B, D, Fr, p('dy'), dy.ld, dy.s, p('gates'), g.ld, g.s,
             p('hout'), o.ld, o.s, p('h0'), p('whh'), p('whht'), p('dgh'), p('dghlp'), p('dgi'),
             p('dgilp'), p('bsum'), d.ld, d.s, p('ddir0'), wk.data_ptr() if nb else None, nb, st)
    else:
        gl = w['dghlp'] if lp else w['dgh']
        other = _work(B * D * 4, t.device)
        ddir = [p('ddir0'), other.data_ptr()]
        for s in reversed(range(Fr)):
            nxt = s + 1 < Fr
            hp, ldhp = (o.ptr(s - 1), o.ld) if s else (p('h0'), D)
            call('srnn_gru_cell_bwd', dc, B, D, dy.ptr(s), dy.ld, gl.ptr(s + 1) if nxt else None,
                 gl.ld, ddir[(s + 1) % 2] if nxt else None, p('whh'), p('whht'), g.ptr(s), g.ld, hp,
                 ldhp, d.ptr(s), d.ld, p('dghlp', s), d.ld, w['dgi'].ptr(s), d.ld, ddir[s % 2], st)
    return works
