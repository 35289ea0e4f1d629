"""Exact-arithmetic cases for the sample-level MLP's kernels and the glue kernels: builders,
CPU evaluators and checkers of the conformance sweep (the method of gemm_cases.py, extended).

None of these kernels contains a transcendental, so with small-integer operands and dyadic
constants every order of summation gives the same bits.  An fp32 output must equal the float64
(or int64) reference bit for bit and a bf16 output its round-to-nearest-even; -0.0 is read as
+0.0.  Each builder states its exactness precondition as an assert.

Placement.  Every operand and output is a gemm_cases.Window: guard rows before and after, row
padding, a canary (a quiet NaN) in every element that is not the operand.  Index streams are
IndexWindow: int64 rows `ld` apart whose window starts `xoff` into the row; every other
element holds 1 << 40, an out-of-range value (its low 32 bits are zero, so a kernel that
strayed onto it would gather entry 0 -- a wrong result, not a wild address).

A built case `t` holds t.w (name -> window), t.outs (names of the output windows),
t.want (name -> expected bits, shaped as Window.read()) and t.ref (the float64 references).
check(t) compares every output and every canary; untouched(t) is the refusal's check.

Plain helper module (no fixtures): test_cpu_mlp_cases.py proves the cases, the GPU test runs
them.
"""
import dataclasses
import types

import torch

from gemm_cases import (CANARY16, CANARY32, DTYPES, PLACEMENTS, Window, _canary, _ints,
                        _outside_report, pack_bits)

XCANARY = 1 << 40
KIB160 = 160 * 1024


def cdiv(a, b):
    return -(-a // b)


class IndexWindow:
    """rows x cols int64 indices, rows `ld` apart, the window `xoff` into each row, inside a
    buffer that holds XCANARY everywhere else (guard rows before and after)."""

    def __init__(self, rows, cols, device, xoff=0, ld=None):
        self.rows, self.cols, self.xoff = rows, cols, xoff
        self.ld = xoff + cols + 5 if ld is None else ld
        assert self.ld >= xoff + cols
        self.front = 2 * self.ld
        self.buf = torch.full((self.front + max(rows, 1) * self.ld + 2 * self.ld,), XCANARY,
                              dtype=torch.int64, device=device)
        r = torch.arange(rows).view(-1, 1) * self.ld
        self.index = (self.front + xoff + r + torch.arange(cols).view(1, -1)).reshape(-1)
        self.before = None

    def fill(self, values):
        self.buf[self.index.to(self.buf.device)] = values.reshape(-1).to(self.buf)

    def read(self):
        return self.buf[self.index.to(self.buf.device)].view(self.rows, self.cols)

    def view(self):
        """The buffer from row 0's start (pass with ldx = ld and xoff)."""
        return self.buf[self.front:]

    def snapshot(self):
        self.before = self.buf.clone()

    def unchanged(self):
        return torch.equal(self.buf, self.before)

    def outside_ok(self):
        keep = torch.ones(self.buf.numel(), dtype=torch.bool, device=self.buf.device)
        keep[self.index.to(self.buf.device)] = False
        return bool((self.buf[keep] == XCANARY).all())


def _gen(*key):
    s = 0
    for k in key:
        s = (s * 1000003 + (k if isinstance(k, int) else sum(map(ord, str(k))))) % (1 << 61)
    return torch.Generator().manual_seed(s)


def _draw(gen, shape, lo, hi):
    return torch.randint(lo, hi + 1, tuple(shape), generator=gen).double()


def bits_of(ref, dtype):
    """A float64 reference as the integers of its `dtype` form (fp32: must be exact; bf16:
    round-to-nearest-even of the exact fp32), -0.0 read as +0.0."""
    r32 = ref.to(torch.float32)
    assert torch.equal(r32.double(), ref.double()), 'reference is not exact in fp32'
    return _ints((r32 + 0.0).to(dtype) + 0.0)


def _win(dtype, rows, cols, place, device, ld=None):
    return Window(dtype, rows, cols, place, device, ld=ld)


def _finish(t):
    """Snapshot the inputs; outputs that are also inputs (t.inout) keep their fill."""
    for k, x in t.w.items():
        if k not in t.outs:
            x.snapshot()
    return t


def _got_bits(x):
    v = x.read().cpu()
    return _ints(v + 0.0) if v.is_floating_point() else v


def check(t):
    """None when every output window holds its expected bits, every canary around every
    window is intact and no input changed; else the report, naming the first wrong element
    (index, got, want) or the first changed canary."""
    bad = []
    for k in t.outs:
        x = t.w[k]
        got, want = _got_bits(x), t.want[k]
        diff = got != want
        if bool(diff.any()):
            i = tuple(int(v) for v in diff.nonzero()[0])
            bad.append('inside the %s window: %d of %d elements differ, first at (row %d, col %d):'
                       ' got 0x%x, want 0x%x' % (k, int(diff.sum()), diff.numel(), i[1], i[2],
                                                 int(got[i]) & 0xffffffff,
                                                 int(want[i]) & 0xffffffff))
        if not x.outside_ok():
            bad.append(_outside_report(x, k))
    for k, x in t.w.items():
        if k not in t.outs and not x.unchanged():
            bad.append('input buffer %s was written' % k)
    return '%s: %s' % (t.case.id, '; '.join(bad)) if bad else None


def all_canary(x):
    return bool((_ints(x.buf) == _canary(x.dtype)).all())


def untouched(t, names=None):
    """None when the named output windows (default: the pure outputs) are canary throughout
    and no input changed; else the report."""
    for k in (t.outs if names is None else names):
        if k in t.inout:
            if not t.w[k].unchanged():
                return '%s: %s was written' % (t.case.id, k)
        elif not all_canary(t.w[k]):
            return '%s: %s' % (t.case.id, _outside_report(_everything_outside(t.w[k]), k))
    for k, x in t.w.items():
        if k not in t.outs and not x.unchanged():
            return '%s: input buffer %s was written' % (t.case.id, k)
    return None


def _everything_outside(x):
    y = types.SimpleNamespace(buf=x.buf, dtype=x.dtype, front=x.front, stride=x.stride, ld=x.ld,
                              index=torch.zeros(0, dtype=torch.int64))
    return y


def _ns(c, device):
    return types.SimpleNamespace(case=c, device=device, w={}, outs=[], inout=[], want={}, ref={})


# ------------------------------------------------------------------------------ L1 gather
# a1 = relu(upper + sum_k Tab[k][x[b, xoff + t + k]]).  Table entries are integers in [-3, 3]
# and upper holds integers in [-16, 16]: with FS0 <= 32 every partial sum is an integer of
# magnitude <= 112 < 256, exact in fp32 and in bf16 in any order.
L1L_NT = 1024


@dataclasses.dataclass(frozen=True)
class L1Case:
    dtype: str                  # table and a1
    udtype: str                 # upper
    B: int
    Tl: int
    D: int
    FS0: int = 16
    Q: int = 256
    places: tuple = ()          # (('upper', 'pad8'), ...): the rest is 'tight'
    xoff: int = 3
    bits: str = ''              # '': srnn_mlp_l1; 'row' / 'grouped': srnn_mlp_l1_bits
    env: tuple = ()

    def placement(self, k):
        return dict(self.places).get(k, 'tight')

    @property
    def id(self):
        s = 'l1-%s.%s-%dx%dx%d-fs%d-q%d-x%d' % (self.dtype, self.udtype, self.B, self.Tl, self.D,
                                                 self.FS0, self.Q, self.xoff)
        for k, v in self.places:
            s += '-%s.%s' % (k, v)
        if self.bits:
            s += '-bits_' + self.bits
        for k, v in self.env:
            s += '-%s=%s' % (k.replace('SRNN_', ''), v)
        return s


def l1case(dtype, udtype, B, Tl, D, FS0=16, Q=256, places=None, env=None, **kw):
    return L1Case(dtype, udtype, B, Tl, D, FS0, Q, tuple(sorted((places or {}).items())),
                  env=tuple(sorted((env or {}).items())), **kw)


def l1_route(c):
    """The kernel that serves this case, 'lds', 'xcd' or 'generic': stated here independently
    of the library, whose l1_plan (csrc/mlp_plan.cpp) test_cpu_mlp_plan.py holds to it."""
    es, ue = (4 if c.dtype == 'f32' else 2), (4 if c.udtype == 'f32' else 2)
    nrows = c.B * c.Tl
    pu, po = PLACEMENTS[c.placement('upper')], PLACEMENTS[c.placement('out')]
    ldu, ldo = c.D + pu[0], c.D + po[0]
    al = pu[1] == 0 and po[1] == 0 and PLACEMENTS[c.placement('tab')][1] == 0
    if es == 2 and ue == 2:
        WP = (c.Tl + c.FS0 - 1 + 4 + 15) & ~15
        if (c.FS0 == 16 and c.Q == 256 and c.D % 16 == 0 and c.D // 16 <= 256 and
                16 * 256 * 32 + 2 * WP <= KIB160 and c.Tl <= 4 * (L1L_NT // 2) and
                WP <= 2 * L1L_NT and nrows >= 4096 and ldu % 8 == 0 and ldo % 8 == 0 and al and
                dict(c.env).get('SRNN_L1_LDS', '1') != '0'):
            return 'lds'
    if (c.D % 128 == 0 and nrows >= 4096 and (ldu * ue) % 16 == 0 and (ldo * es) % 16 == 0 and al):
        return 'xcd'
    return 'generic'


def build_l1(c, device='cpu'):
    assert c.FS0 <= 32 and c.D % 4 == 0 and c.xoff in (0, 3)
    assert c.placement('tab') in ('tight', 'off1'), 'the table has no leading dimension'
    assert not c.bits or (c.dtype == c.udtype == 'bf16' and c.D % 16 == 0)
    assert c.bits != 'grouped' or c.D % 64 == 0
    dt, du = DTYPES[c.dtype], DTYPES[c.udtype]
    rows, W = c.B * c.Tl, c.Tl + c.FS0 - 1
    t = _ns(c, device)
    for attempt in range(32):               # tiny cases: a draw whose ReLU clamps about half
        gen = _gen('l1', c.B, c.Tl, c.D, c.FS0, c.Q, attempt)
        tab = _draw(gen, (c.FS0, c.Q, c.D), -3, 3)
        x = torch.randint(0, c.Q, (c.B, W), generator=gen)
        upper = _draw(gen, (rows, c.D), -16, 16)
        pre = upper.clone()
        for k in range(c.FS0):
            pre += tab[k][x[:, k:k + c.Tl].reshape(-1)]
        share = float((pre <= 0).double().mean())
        if 0.3 <= share <= 0.7:
            break
    assert 0.3 <= share <= 0.7, 'case %s: the ReLU clamps %.2f of the outputs' % (c.id, share)
    assert float(upper.abs().max()) + 3 * c.FS0 <= 112 < 256            # exact in bf16 and fp32
    t.ref['a1'] = pre.clamp_min(0.0)
    t.values = dict(tab=tab, x=x, upper=upper)
    t.w['tab'] = _win(dt, c.FS0 * c.Q, c.D, c.placement('tab'), device)
    t.w['tab'].fill(tab)
    t.w['x'] = IndexWindow(c.B, W, device, xoff=c.xoff)
    t.w['x'].fill(x)
    t.w['upper'] = _win(du, rows, c.D, c.placement('upper'), device)
    t.w['upper'].fill(upper)
    t.w['out'] = _win(dt, rows, c.D, c.placement('out'), device)
    t.outs = ['out']
    t.want['out'] = bits_of(t.ref['a1'], dt).view(1, rows, c.D)
    if c.bits:
        ng = c.D // 16
        words = pack_bits(t.ref['a1'] > 0)                              # (1, rows, ng)
        if c.bits == 'row':
            t.w['bits'] = _win(torch.int16, rows, ng, 'tight', device, ld=ng + 3)
            t.want['bits'] = words
        else:                                                           # [column group][row]
            t.w['bits'] = _win(torch.int16, ng, rows, 'tight', device)
            t.want['bits'] = words.transpose(1, 2).contiguous()
        t.outs.append('bits')
    return _finish(t)


def eval_l1(t):
    """fp32 on the CPU from the placed operands, taps in reverse and upper last (the kernels
    start from upper and walk the taps upwards), written into the output windows."""
    c, w = t.case, t.w
    tab = w['tab'].read().cpu().float().view(c.FS0, c.Q, c.D)
    x = w['x'].read().cpu()
    acc = torch.zeros(c.B * c.Tl, c.D, dtype=torch.float32)
    for k in reversed(range(c.FS0)):
        acc += tab[k][x[:, k:k + c.Tl].reshape(-1)]
    acc = (acc + w['upper'].read().cpu().float().view(-1, c.D)).clamp_min(0.0)
    w['out'].fill(acc.to(DTYPES[c.dtype]))
    if c.bits:
        words = pack_bits(acc.to(DTYPES[c.dtype]).float() > 0)
        w['bits'].fill(words if c.bits == 'row' else words.transpose(1, 2))
    return acc


# ------------------------------------------------------------------------------ dTab
# dTab[q][k][:] = sum over (b, t) with x[b, xoff + t + k] == q of da[b, t, :], and
# colsum[j * D + c] = sum over b and t = j (mod FS0) of da[b, t, c].  da holds integers in
# [-3, 3] times 2^-8, so the 2^-40 fixed-point terms are exact integers and every sum is exact.
@dataclasses.dataclass(frozen=True)
class DtabCase:
    dtype: str
    out: str
    B: int
    Tl: int
    D: int
    FS0: int = 16
    Q: int = 256
    dist: str = 'uniform'       # 'uniform' / 'runs' / 'skew' (60 % one value) / 'few' (4 values)
    pad: int = 0                # ldda = D + pad
    xoff: int = 3
    entry: int = 4              # srnn_mlp_dtab{'', 2, 3, 4}
    amax: bool = False          # amax_in given
    blk: bool = False           # the column-blocked copy of da given
    positive: bool = False      # da in [0, 3] 2^-8: sums large enough to need bf16 rounding
    env: tuple = ()

    @property
    def id(self):
        s = 'dtab%d-%s>%s-%dx%dx%d-fs%d-q%d-%s-ld+%d-x%d' % (
            self.entry, self.dtype, self.out, self.B, self.Tl, self.D, self.FS0, self.Q, self.dist,
            self.pad, self.xoff)
        s += ('-amax' if self.amax else '') + ('-blk' if self.blk else '')
        s += '-pos' if self.positive else ''
        for k, v in self.env:
            s += '-%s=%s' % (k.replace('SRNN_DTAB_', ''), v)
        return s


def dcase(dtype, out, B, Tl, D, FS0=16, Q=256, env=None, **kw):
    return DtabCase(dtype, out, B, Tl, D, FS0, Q, env=tuple(sorted((env or {}).items())), **kw)


def pos_lds_bytes(Q, Tl):
    WPB = (Tl + 15 + 31) & ~15
    return Q * 16 * 4 * 8 + 4 * 16 * 8 + 16 * WPB


def pk_lds_bytes(Q, Tl):
    WPB = (Tl + 15 + 31) & ~15
    return Q * 2 * 16 * 8 + 4 * 16 * 8 + 16 + 16 * 2 * WPB


def dtab_route(c):
    """The path srnn_mlp_dtab4 takes, 'packed', 'direct', 'posws' (position-major with
    workspace), 'generic<cw>' or 'empty': stated here independently of the library, whose
    dtab_plan (csrc/mlp_plan.cpp) test_cpu_mlp_plan.py holds to it."""
    env = dict(c.env)
    off = lambda k: env.get(k, '1')[:1] == '0'                          # noqa: E731
    n = c.B * c.Tl
    if (c.dtype == 'bf16' and c.out == 'bf16' and c.FS0 == 16 and c.Q == 256 and c.D % 8 == 0 and
            (c.D + c.pad) % 8 == 0 and cdiv(c.D, 4) >= 192 and pk_lds_bytes(c.Q, c.Tl) <= KIB160 and
            pos_lds_bytes(c.Q, c.Tl) <= KIB160 and n > 0 and not off('SRNN_DTAB_PACK')):
        return 'packed'
    if c.FS0 == 16 and pos_lds_bytes(c.Q, c.Tl) <= KIB160 and n > 0 and not off('SRNN_DTAB_POS'):
        return 'direct' if cdiv(c.D, 4) >= 192 else 'posws'
    if n <= 0:
        return 'empty'
    W, cw = c.Tl + c.FS0 - 1, 4
    while cw > 1 and (c.Q * c.FS0 * cw * 8 + W > KIB160 or c.FS0 * cw > 1024):
        cw //= 2
    return 'generic%d' % cw


def dtab_indices(c, gen):
    W = c.Tl + c.FS0 - 1
    x = torch.randint(0, c.Q, (c.B, W), generator=gen)
    if c.dist == 'runs':                    # runs of one value, 1 to 40 positions long
        flat, i = x.reshape(-1), 0
        while i < flat.numel():
            n = int(torch.randint(1, 41, (1,), generator=gen))
            flat[i:i + n] = flat[i]
            i += n
    elif c.dist == 'skew':
        x = torch.where(torch.rand((c.B, W), generator=gen) < 0.6,
                        torch.full_like(x, min(131, c.Q - 1)), x)
    elif c.dist == 'few':
        x = torch.tensor([0, 63, 64, 255])[torch.randint(0, 4, (c.B, W), generator=gen)] % c.Q
    else:
        assert c.dist == 'uniform'
    return x


def packed_exponent(amax, cmax):
    """The packed kernel's scale exponent: e = min(floor(log2(2^30 / (amax cmax))), 40)."""
    import math
    return min(math.frexp(1073741824.0 / (amax * cmax))[1] - 1, 40)


def build_dtab(c, device='cpu'):
    assert c.Q <= 256 and c.entry in (1, 2, 3, 4)
    assert not (c.amax and c.entry < 3) and not (c.blk and c.entry < 4)
    dt, do = DTYPES[c.dtype], DTYPES[c.out]
    rows, W, n = c.B * c.Tl, c.Tl + c.FS0 - 1, c.Q * c.FS0 * c.D
    gen = _gen('dtab', c.B, c.Tl, c.D, c.FS0, c.Q, c.dist)
    t = _ns(c, device)
    x = dtab_indices(c, gen)
    ints = _draw(gen, (rows, c.D), 0 if c.positive else -3, 3)
    da = ints * 2.0 ** -8
    route = dtab_route(c)
    if route == 'packed':
        # the packed form's own precondition: its terms round(da 2^e) are exact integers and
        # every 32-bit sum stays below 2^30.  cmax counts the window positions only.
        cmax = int(torch.bincount(x.reshape(-1), minlength=c.Q).max())
        amax = float(da.abs().max())
        e = packed_exponent(amax, cmax)
        assert e >= 8 and 3 * cmax * 2 ** (e - 8) < 2 ** 30, 'case %s: packed form inexact' % c.id
        t.e, t.cmax = e, cmax
    tab = torch.zeros(c.Q, c.FS0, c.D, dtype=torch.float64)
    for k in range(c.FS0):
        tab[:, k, :].index_add_(0, x[:, k:k + c.Tl].reshape(-1), da)
    cs = torch.zeros(c.FS0, c.D, dtype=torch.float64)
    if rows:
        j = (torch.arange(c.Tl) % c.FS0).repeat(c.B)
        cs.index_add_(0, j, da)
    # exactness: every sum is an integer multiple of 2^-8 below 2^24 2^-8
    assert float(tab.abs().max()) * 256 < 2 ** 24 and float(cs.abs().max()) * 256 < 2 ** 24
    t.ref.update(dtab=tab, colsum=cs)
    t.values = dict(x=x, da=da)
    t.route = route
    t.colsum_done = c.entry >= 2 and route in ('packed', 'direct')
    t.w['da'] = _win(dt, rows, c.D, 'tight', device, ld=c.D + c.pad)
    t.w['da'].fill(da)
    t.w['x'] = IndexWindow(c.B, W, device, xoff=c.xoff)
    t.w['x'].fill(x)
    if c.amax:
        t.w['amax'] = _win(torch.float32, 1, 1, 'tight', device)       # max |da| as float bits
        t.w['amax'].fill(da.abs().max().view(1, 1, 1) if rows else torch.zeros(1, 1, 1))
    if c.blk:
        assert c.D % 4 == 0
        t.w['blk'] = _win(dt, (c.D // 4) * rows, 4, 'tight', device)   # blk[D / 4][B Tlen][4]
        t.w['blk'].fill(da.view(rows, c.D // 4, 4).permute(1, 0, 2))
    t.w['dtab'] = _win(do, c.Q * c.FS0, c.D, 'tight', device)
    t.want['dtab'] = bits_of(tab, do).view(1, c.Q * c.FS0, c.D)
    t.outs = ['dtab']
    if c.entry >= 2:
        t.w['colsum'] = _win(torch.float32, c.FS0, c.D, 'tight', device)
        t.want['colsum'] = bits_of(cs, torch.float32).view(1, c.FS0, c.D)
        t.outs.append('colsum')
        t.w['colsum'].snapshot()               # all canary: what a call that skips it leaves
    t.work_elems = n + 64                   # int64 scratch (>= Q FS0 D 8 bytes), not an operand
    return _finish(t)


def eval_dtab(t):
    """fp32 on the CPU from the placed operands, rows and taps in reverse order."""
    c, w = t.case, t.w
    da = w['da'].read().cpu().float().view(-1, c.D).flip(0)
    x = w['x'].read().cpu()
    tab = torch.zeros(c.Q, c.FS0, c.D, dtype=torch.float32)
    for k in reversed(range(c.FS0)):
        tab[:, k, :].index_add_(0, x[:, k:k + c.Tl].reshape(-1).flip(0), da)
    w['dtab'].fill(tab.to(DTYPES[c.out]))
    cs = torch.zeros(c.FS0, c.D, dtype=torch.float32)
    if da.numel():
        cs.index_add_(0, (torch.arange(c.Tl) % c.FS0).repeat(c.B).flip(0), da)
    if 'colsum' in w and t.colsum_done:
        w['colsum'].fill(cs)
    return tab, cs


def check_dtab(t, done):
    """check(), with the column sums compared only when the call reported them written
    (`done`, which must be what the route implies); otherwise their window stays canary."""
    if 'colsum' not in t.w:
        return check(t)
    if bool(done) != t.colsum_done:
        return '%s: colsum_done = %d on the %s route' % (t.case.id, done, t.route)
    if done:
        return check(t)
    outs = t.outs
    try:
        t.outs = ['dtab']
        r = check(t)                        # (colsum then counts as an input: unchanged)
    finally:
        t.outs = outs
    return r


# ------------------------------------------------------------------------------ output backward
# dz and wt hold integers in [-3, 3], a2 integers in [0, 3] with about half zeros (bf16).
OB_Q = 256


@dataclasses.dataclass(frozen=True)
class OutBwdCase:
    M: int
    D: int
    ranges: int
    want_db: bool = True
    off1: str = ''              # an operand handed over 2 bytes past a 16-byte boundary

    @property
    def id(self):
        return 'outbwd-%dx%d-r%d%s%s' % (self.M, self.D, self.ranges,
                                         '' if self.want_db else '-nodb',
                                         '-%s.off1' % self.off1 if self.off1 else '')


def out_bwd_served(c):
    """The contract of srnn_mlp_out_bwd: Q = 256, D % 128 == 0, M % 256 == 0, 16-byte bases."""
    return c.M > 0 and c.M % 256 == 0 and c.D > 0 and c.D % 128 == 0 and not c.off1


def build_out_bwd(c, device='cpu'):
    M, D, Q = c.M, c.D, OB_Q
    assert 9 * M < 2 ** 24 and 9 * Q < 2 ** 24
    gen = _gen('outbwd', M, D)
    bf = torch.bfloat16
    dz = _draw(gen, (M, Q), -3, 3)
    a2 = _draw(gen, (M, D), 0, 3) * (torch.rand((M, D), generator=gen) < 0.67).double()
    zeros = float((a2 == 0).double().mean())
    assert 0.4 <= zeros <= 0.6, zeros
    wt = _draw(gen, (D, Q), -3, 3)
    t = _ns(c, device)
    da2 = torch.where(a2 > 0, dz @ wt.t(), torch.zeros((), dtype=torch.float64))
    stored = da2.float().to(bf).double()                                # RNE bf16 of the product
    nblk = max(M // 128, 1)
    csp = stored[:nblk * 128].view(nblk, -1, D).sum(1) if M >= 128 else torch.zeros(1, D).double()
    assert float(stored.abs().sum(0).max()) < 2 ** 24                   # integer sums, exact
    t.ref.update(da2=da2, dW=dz.t() @ a2, db=dz.sum(0), csp=csp, db_hid=stored.sum(0))
    t.values = dict(dz=dz, a2=a2, wt=wt)
    for k, v in (('dz', dz), ('a2', a2), ('wt', wt)):
        t.w[k] = _win(bf, v.shape[0], v.shape[1], 'off1' if c.off1 == k else 'tight', device)
        t.w[k].fill(v)
    t.w['da2'] = _win(bf, M, D, 'off1' if c.off1 == 'da2' else 'tight', device)
    t.w['dW'] = _win(torch.float32, Q, D, 'tight', device)
    t.w['csp'] = _win(torch.float32, nblk, D, 'tight', device)
    t.outs = ['da2', 'dW', 'csp']
    t.want.update(da2=bits_of(da2, bf).view(1, M, D), dW=bits_of(t.ref['dW'], torch.float32).view(1, Q, D),
                  csp=bits_of(csp, torch.float32).view(1, nblk, D))
    if c.want_db:
        t.w['db'] = _win(torch.float32, 1, Q, 'tight', device)
        t.want['db'] = bits_of(t.ref['db'], torch.float32).view(1, 1, Q)
        t.outs.append('db')
    return _finish(t)


def eval_out_bwd(t):
    """fp32 on the CPU: the reductions run with k (and the rows) reversed."""
    c, w = t.case, t.w
    dz, a2, wt = (w[k].read().cpu().float()[0] for k in ('dz', 'a2', 'wt'))
    da2 = torch.where(a2 > 0, dz.flip(1) @ wt.flip(1).t(), torch.zeros(()))
    stored = da2.to(torch.bfloat16)
    w['da2'].fill(stored)
    w['dW'].fill(dz.flip(0).t() @ a2.flip(0))
    nblk = w['csp'].rows
    w['csp'].fill(stored.float().flip(0)[:nblk * 128].view(nblk, -1, c.D).sum(1).flip(0)
                  if c.M >= 128 else torch.zeros(1, c.D))
    if c.want_db:
        w['db'].fill(dz.flip(0).sum(0))
    return da2


# ------------------------------------------------------------------------------ loss head
NLL_TARGETS = (0, 63, 64, 127, 255)


@dataclasses.dataclass(frozen=True)
class NllCase:
    op: str                     # 'bwd' / 'fwd'
    B: int
    Tl: int
    Q: int = 256
    place: str = 'tight'        # of dlogp (bwd) / logp (fwd)
    gmul: bool = False
    ldt_extra: int = 3

    @property
    def id(self):
        return 'nll_%s-%dx%d-q%d-%s%s' % (self.op, self.B, self.Tl, self.Q, self.place,
                                          '-gmul' if self.gmul else '')


def nll_bwd_route(c):
    pad, off = PLACEMENTS[c.place]
    return 'q256' if c.Q == 256 and (c.Q + pad) % 4 == 0 and off == 0 else 'generic'


def build_nll(c, device='cpu'):
    rows, Q = c.B * c.Tl, c.Q
    gen = _gen('nll', c.op, c.B, c.Tl, Q)
    t = _ns(c, device)
    tg = torch.randint(0, Q, (rows,), generator=gen)
    edge = torch.tensor([v for v in NLL_TARGETS if v < Q])
    tg[:min(rows, edge.numel())] = edge.roll(rows % edge.numel())[:rows]
    t.w['target'] = IndexWindow(c.B, c.Tl, device, xoff=0, ld=c.Tl + c.ldt_extra)
    t.w['target'].fill(tg)
    t.values = dict(target=tg)
    if c.op == 'bwd':
        t.gscale = 0.375                                                # dyadic
        g = t.gscale * (0.5 if c.gmul else 1.0)
        if c.gmul:
            t.w['gmul'] = _win(torch.float32, 1, 1, 'tight', device)
            t.w['gmul'].fill(torch.full((1, 1, 1), 0.5))
        ref = torch.zeros(rows, Q, dtype=torch.float64)
        ref[torch.arange(rows), tg] = -g
        t.ref['dlogp'] = ref
        t.w['dlogp'] = _win(torch.float32, rows, Q, c.place, device)
        t.want['dlogp'] = bits_of(ref, torch.float32).view(1, rows, Q)
        t.outs = ['dlogp']
    else:
        logp = _draw(gen, (rows, Q), -64, 0)                            # integer-valued
        t.values['logp'] = logp
        t.w['logp'] = _win(torch.float32, rows, Q, c.place, device)
        t.w['logp'].fill(logp)
        ref = -logp[torch.arange(rows), tg]
        t.ref['loss'] = ref
        t.w['loss'] = _win(torch.float32, 1, rows, 'tight', device)
        t.want['loss'] = bits_of(ref, torch.float32).view(1, 1, rows)
        t.outs = ['loss']
    return _finish(t)


def eval_nll(t):
    c, w = t.case, t.w
    tg = w['target'].read().cpu().reshape(-1)
    rows = tg.numel()
    if c.op == 'bwd':
        g = torch.tensor(t.gscale, dtype=torch.float32)
        if c.gmul:
            g = g * w['gmul'].read().cpu().view(())
        v = torch.where(torch.arange(c.Q).view(1, -1) == tg.view(-1, 1), -g, torch.zeros(()))
        w['dlogp'].fill(v)
    else:
        v = -w['logp'].read().cpu()[0][torch.arange(rows), tg]
        w['loss'].fill(v)
    return v


# ------------------------------------------------------------------------------ glue
# Operands are integers in [-3, 3] (casts: integers up to 2^12, so a bf16 store must round),
# alpha and beta are dyadic: every result is exact in fp32 in any order.
@dataclasses.dataclass(frozen=True)
class GlueCase:
    op: str                     # the entry point, e.g. 'srnn_gather_rows'
    rows: int
    cols: int
    out: str = 'f32'
    src: str = 'f32'
    place: str = 'pad1'         # of every strided operand
    alpha: float = 1.0
    beta: float = 1.0
    accumulate: bool = False
    alias: bool = False         # axpby: out is a
    perm: tuple = (0, 1, 2)
    d0: int = 1                 # permute3: (d0, rows, cols)

    @property
    def id(self):
        s = '%s-%dx%d-%s>%s-%s' % (self.op.replace('srnn_', ''), self.rows, self.cols, self.src,
                                   self.out, self.place)
        if self.op == 'srnn_permute3':
            s += '-d%d-p%d%d%d' % ((self.d0,) + self.perm)
        if (self.alpha, self.beta) != (1.0, 1.0):
            s += '-a%g-b%g' % (self.alpha, self.beta)
        return s + ('-acc' if self.accumulate else '') + ('-alias' if self.alias else '')


GLUE_SHAPES = ((1, 1), (3, 5), (37, 70), (0, 8), (70001, 3))
MULTI_SIZES = [1, 3, 0, 7, 64, 1000, 2049, 0, 4096, 5003] * 9          # 90 tensors, 18 empty


def _indices(gen, n, trows):
    """n row indices into trows rows: duplicates, and rows that never occur (the odd ones)."""
    return torch.randint(0, max(1, cdiv(trows, 2)), (n,), generator=gen) * 2 % max(trows, 1)


def flat_window(dtype, ranges, total, device):
    """A 1-D window whose operand is the union of `ranges` [(offset, n), ...] of `total`
    elements: the gaps between the tensors of a packed bucket count as canaries."""
    x = Window(dtype, 1, max(total, 1), 'tight', device)
    idx = [torch.arange(o, o + n) for o, n in ranges if n > 0]
    x.index = x.front + (torch.cat(idx) if idx else torch.zeros(0, dtype=torch.int64))
    x.cols = int(x.index.numel())
    return x


def build_glue(c, device='cpu'):
    f32 = torch.float32
    do, ds = DTYPES[c.out], DTYPES[c.src]
    R, C, op = c.rows, c.cols, c.op
    gen = _gen(op, R, C, c.out, c.src)
    t = _ns(c, device)
    w = t.w

    def put(name, dtype, rows, cols, vals, place=c.place, out=False, ld=None):
        w[name] = _win(dtype, rows, cols, place, device, ld=ld)
        if vals is not None:
            w[name].fill(vals)
        if out:
            t.outs.append(name)
            if vals is not None:
                t.inout.append(name)

    def want(name, ref, dtype):
        t.ref[name] = ref
        t.want[name] = bits_of(ref.contiguous(), dtype).reshape(w[name].nb, w[name].rows, w[name].cols)

    if op == 'srnn_gather_rows':
        trows = max(2, R // 2 + 3) if R < 1000 else 41
        tab, idx = _draw(gen, (trows, C), -3, 3), _indices(gen, R, trows)
        put('table', f32, trows, C, tab)
        w['idx'] = IndexWindow(1, R, device)
        w['idx'].fill(idx)
        put('out', do, R, C, None, out=True)
        want('out', tab[idx], do)
    elif op in ('srnn_scatter_add_rows', 'srnn_index_add_rows'):
        trows = max(2, R // 2 + 3) if R < 1000 else 7
        tab, idx, src = _draw(gen, (trows, C), -3, 3), _indices(gen, R, trows), _draw(gen, (R, C), -3, 3)
        assert 3 + 3 * R < 2 ** 24
        put('src', f32, R, C, src)
        w['idx'] = IndexWindow(1, R, device)
        w['idx'].fill(idx)
        put('table', f32, trows, C, tab, out=True)
        want('table', tab.clone().index_add_(0, idx, src), f32)
        t.values = dict(tab=tab, idx=idx, src=src)
    elif op == 'srnn_add_bcast_rows':                                   # x (B, F, D) dense
        F = 2
        x, v = _draw(gen, (R * F, C), -3, 3), _draw(gen, (R, C), -3, 3)
        put('v', f32, R, C, v)
        put('x', f32, R * F, C, x, place='tight', out=True)
        want('x', x + v.repeat_interleave(F, 0), f32)
    elif op == 'srnn_axpby':                                            # flat, n = rows * cols
        n = R * C
        a, b = _draw(gen, (1, n), -3, 3), _draw(gen, (1, n), -3, 3)
        assert c.alpha * 8 == int(c.alpha * 8) and c.beta * 8 == int(c.beta * 8)
        put('b', f32, 1, n, b, place='tight')
        put('a', f32, 1, n, a, place='tight', out=c.alias)
        if not c.alias:
            put('out', f32, 1, n, None, place='tight', out=True)
        want('a' if c.alias else 'out', c.alpha * a + c.beta * b, f32)
    elif op == 'srnn_segsum':                                           # src (B F, D) -> (B, D)
        F = 3
        src = _draw(gen, (R * F, C), -3, 3)
        put('src', f32, R * F, C, src)
        put('out', f32, R, C, None, place='tight', out=True)
        want('out', src.view(R, F, C).sum(1), f32)
    elif op == 'srnn_colsum':
        src = _draw(gen, (R, C), -3, 3)
        assert 3 * R * abs(c.alpha) + 3 < 2 ** 24
        put('src', ds, R, C, src)
        old = _draw(gen, (1, C), -3, 3) if c.accumulate else None
        put('out', f32, 1, C, old, place='tight', out=True)
        want('out', (old if c.accumulate else 0.0) + c.alpha * src.sum(0, keepdim=True), f32)
        nrb = max(1, min((R + 63) // 64, 2048 // max(1, (C + 63) // 64)))
        t.work_elems = nrb * C + 256
    elif op == 'srnn_copy2d':
        src = _draw(gen, (R, C), -4099, 4099)
        if ds == torch.bfloat16:
            src = src.float().to(ds).double()
        put('src', ds, R, C, src)
        put('out', do, R, C, None, out=True)
        want('out', src, do)
    elif op == 'srnn_permute3':                                         # dense (d0, R, C)
        d = (c.d0, R, C)
        src = _draw(gen, d, -3, 3)
        od = [d[p] for p in c.perm]
        old = _draw(gen, od, -3, 3) if c.accumulate else None
        put('src', f32, d[0] * d[1], d[2], src, place='tight')
        put('out', do, od[0] * od[1], od[2], old, place='tight', out=True)
        want('out', (old if c.accumulate else 0.0) + src.permute(*c.perm), do)
        t.dims = d
    elif op in ('srnn_pack_grads', 'srnn_cast_multi'):
        sizes = MULTI_SIZES
        assert len(sizes) > 64 and 0 in sizes
        t.sizes, t.offs, t.null, off, vals = sizes, [], [], 0, []
        for i, n in enumerate(sizes):
            null = op == 'srnn_pack_grads' and i % 5 == 1               # a NULL source: zeros
            v = _draw(gen, (1, n), -4099, 4099) * (0.0 if null else 1.0)
            t.null.append(null)
            vals.append(v)
            if not null:
                put('src%d' % i, f32, 1, n, v, place=('tight', 'off1')[i % 2] if n else 'tight')
            t.offs.append(off)
            off = (off + n + 63) // 64 * 64 + (64 if i % 3 == 0 else 0)  # 64-aligned, some gaps
        assert all(o % 64 == 0 for o in t.offs)
        if op == 'srnn_pack_grads':
            w['flat'] = flat_window(do, list(zip(t.offs, sizes)), off, device)
            t.outs.append('flat')
            want('flat', torch.cat(vals, 1), do)
        else:
            for i, n in enumerate(sizes):
                put('dst%d' % i, torch.bfloat16, 1, n, None, place='tight', out=True)
                want('dst%d' % i, vals[i], torch.bfloat16)
    else:
        raise ValueError(op)
    return _finish(t)


def eval_glue(t):
    """The operation in fp32 on the CPU from the placed operands, in another order where there
    is one (rows reversed), written into the output windows."""
    c, w, op = t.case, t.w, t.case.op
    rd = lambda k: w[k].read().cpu().float()[0]                         # noqa: E731
    if op == 'srnn_gather_rows':
        w['out'].fill(rd('table')[w['idx'].read().cpu().view(-1)].to(DTYPES[c.out]))
    elif op in ('srnn_scatter_add_rows', 'srnn_index_add_rows'):
        idx = w['idx'].read().cpu().view(-1)
        w['table'].fill(rd('table').index_add_(0, idx.flip(0), rd('src').flip(0)))
    elif op == 'srnn_add_bcast_rows':
        w['x'].fill(rd('x') + rd('v').repeat_interleave(2, 0))
    elif op == 'srnn_axpby':
        w['a' if c.alias else 'out'].fill(c.beta * rd('b') + c.alpha * rd('a'))
    elif op == 'srnn_segsum':
        w['out'].fill(rd('src').view(c.rows, 3, c.cols).flip(1).sum(1))
    elif op == 'srnn_colsum':
        s = c.alpha * rd('src').flip(0).sum(0, keepdim=True)
        w['out'].fill(rd('out') + s if c.accumulate else s)
    elif op == 'srnn_copy2d':
        w['out'].fill(rd('src').to(DTYPES[c.out]))
    elif op == 'srnn_permute3':
        v = rd('src').view(t.dims).permute(*c.perm)
        w['out'].fill((rd('out').view(v.shape) + v if c.accumulate else v).to(DTYPES[c.out]))
    elif op == 'srnn_pack_grads':
        vals = [torch.zeros(1, n) if t.null[i] else rd('src%d' % i).view(1, n)
                for i, n in enumerate(t.sizes)]
        w['flat'].fill(torch.cat(vals, 1).to(DTYPES[c.out]))
    elif op == 'srnn_cast_multi':
        for i in range(len(t.sizes)):
            w['dst%d' % i].fill(rd('src%d' % i).to(torch.bfloat16))


FAMILIES = {'l1': (build_l1, eval_l1), 'dtab': (build_dtab, eval_dtab),
            'out_bwd': (build_out_bwd, eval_out_bwd), 'nll': (build_nll, eval_nll),
            'glue': (build_glue, eval_glue)}
assert CANARY16 == CANARY32 >> 16
