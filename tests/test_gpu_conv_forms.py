"""GPU: every instantiation of the gather convolution (csrc/conv_gather.hip, hc_conv_gather) at shapes that reach it, with the
instantiation asserted from the kernel trace (tests/_kernel_trace.py).

The host dispatcher picks one of ~22 forms of conv_gather_kernel<MR, NR, WM, WN, BK, FP8, NS, MINB> by shape rules and tile-count
heuristics, so a shape only tests the form it reaches.  Every case here names that form and fails when the dispatch moves.

Reference and bound: bf16-representable operands, torch-CPU fp32 F.conv2d / conv2d_input, checked ELEMENT-WISE

    |y - ref| <= 2^-8 |ref| + 2^-10 A

with A the same convolution of |x| and |w| (+ |resid|): the first term is the bf16 rounding of the output, the second a generous
bound on fp32 accumulation error.  A wrong tile or a swapped channel is off by O(A).  Statistics are checked per channel against
fp64 sums within 2^-12 of the sum of magnitudes.  Every destination is allocated with guard zones on both sides and filled with a
NaN pattern first: every logical element must be written, and nothing outside it.

Default knobs only: the HC_CONV_* variables are read once per process.
"""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F
from torch.nn.grad import conv2d_input

from conftest import rel_l2
from _kernel_trace import launched_gather_form

pytestmark = pytest.mark.gpu

# ------------------------------------------------------------------ the instantiations
BIG256 = (4, 2, 2, 4, 32, False, 4, 1)      # 256 x 256 tile, one workgroup per CU
BIG128 = (4, 2, 1, 8, 32, False, 4, 1)      # 128 x 512 tile (96 < Cout <= 128)
DEEP = (1, 2, 2, 2, 64, False, 3, 2)        # classic 64 x 128 tile, deep-pipeline loop
SHORT32 = (1, 2, 1, 4, 32, False, 2, 4)     # short-loop forms, four workgroups per CU
SHORT64 = (1, 2, 2, 2, 32, False, 2, 4)
SHORT128 = (2, 2, 2, 2, 32, False, 2, 4)


def classic(mr, nr, wm, wn, bk):
    return (mr, nr, wm, wn, bk, False, 2, 2)


def fp8form(mr, nr, wm, wn):
    return (mr, nr, wm, wn, 32, True, 2, 2)


def tile(form):
    """(channel rows, pixel columns) of a form's tile"""
    mr, nr, wm, wn = form[:4]
    return 32 * mr * wm, 32 * nr * wn


# ------------------------------------------------------------------ helpers
GUARD = 4096                 # elements of guard zone on each side of a destination
NAN_BF16 = 0x7fc0            # bf16 quiet NaN, as int16
NAN_FP8 = 0xff               # e4m3fn NaN byte (the kernel saturates to +-448, never writes it)
DEV = "cuda"


def bf16r(t):
    return t.to(torch.bfloat16).float()


def gen(*key):
    return torch.Generator().manual_seed(sum((i + 1) * 7919 * k for i, k in enumerate(key)) % (2 ** 31))


class Guarded:
    """NHWC destination [N][H][W][C] inside a NaN-filled allocation with GUARD elements on each side."""

    def __init__(self, N, Cc, H, W, fp8=False):
        self.n = N * H * W * Cc
        self.fp8 = fp8
        self.shape = (N, Cc, H, W)
        dt = torch.uint8 if fp8 else torch.int16
        self.buf = torch.empty((self.n + 2 * GUARD,), dtype=dt, device=DEV)
        self.reset()
        body = self.buf[GUARD:GUARD + self.n]
        if not fp8:
            body = body.view(torch.bfloat16)
        self.t = body.view(N, H, W, Cc).permute(0, 3, 1, 2)       # logical NCHW, channels_last strides

    def reset(self):
        if self.fp8:
            self.buf.fill_(NAN_FP8)
        else:
            self.buf.fill_(NAN_BF16)

    def check(self, what):
        """every element written, nothing outside; returns the logical NCHW fp32 (bf16 dst) or uint8 (fp8 dst) CPU tensor"""
        pat = NAN_FP8 if self.fp8 else NAN_BF16
        head, tail = self.buf[:GUARD].cpu(), self.buf[GUARD + self.n:].cpu()
        if not self.fp8:
            head, tail = head.to(torch.int32) & 0xffff, tail.to(torch.int32) & 0xffff
        assert bool((head == pat).all()) and bool((tail == pat).all()), (what, "write outside the destination")
        if self.fp8:
            got = self.t.cpu().contiguous()
            assert not bool(((got & 0x7f) == 0x7f).any()), (what, "unwritten (NaN) elements", int(((got & 0x7f) == 0x7f).sum()))
            return got
        got = self.t.float().cpu().contiguous()
        nan = torch.isnan(got)
        assert not bool(nan.any()), (what, "unwritten elements", int(nan.sum()), nan.nonzero()[:4].tolist())
        return got


def check_bound(got, ref, A, what):
    err = (got.double() - ref.double()).abs()
    lim = 2.0 ** -8 * ref.double().abs() + 2.0 ** -10 * A.double()
    bad = err > lim
    if bool(bad.any()):
        i = tuple(bad.nonzero()[0].tolist())
        raise AssertionError("%s: %d of %d elements outside |y - ref| <= 2^-8 |ref| + 2^-10 A; first at %s: got %g ref %g A %g"
                             % (what, int(bad.sum()), bad.numel(), i, float(got[i]), float(ref[i]), float(A[i])))


def check_stats(stats, acc, what):
    """stats: [replicas][2][C] device accumulators of the fp32 results `acc` (logical NCHW)"""
    s = stats.double().cpu().sum(0)
    a = acc.double()
    s1, s2, sa = a.sum((0, 2, 3)), (a * a).sum((0, 2, 3)), a.abs().sum((0, 2, 3))
    assert bool(((s[0] - s1).abs() <= 2.0 ** -12 * sa + 1e-6).all()), (what, "sum", float((s[0] - s1).abs().max()))
    assert bool(((s[1] - s2).abs() <= 2.0 ** -12 * s2 + 1e-6).all()), (what, "sum of squares", float((s[1] - s2).abs().max()))


def act_ref(v, act, slope):
    if act == 0:
        return v
    if act == 1:
        return F.relu(v)
    if act == 2:
        return 0.5 * v * (v + 2).clamp(0, 2)
    if act == 3:
        return torch.where(v > 0, v, slope * v)
    if act == 4:
        return v * torch.tanh(F.softplus(v))
    if act == 5:
        return v * torch.sigmoid(v)
    if act == 6:
        return v.clamp(0, 6)
    raise ValueError(act)


def operands(N, Cin, Cout, H, W, k, seed):
    g = gen(seed, N, Cin, Cout, H, W, k)
    x = bf16r(torch.randn((N, Cin, H, W), generator=g))
    w = bf16r(torch.randn((Cout, Cin, k, k), generator=g) / (Cin * k * k) ** 0.5)
    return g, x, w


def fwd_ref(x, w, stride, pad):
    return F.conv2d(x, w, None, stride, pad), F.conv2d(x.abs(), w.abs(), None, stride, pad)


def launch(d, *args, **kw):
    from holocron_amd.ops import conv as cv
    return launched_gather_form(lambda: cv.launch_conv(d, *args, **kw))


# ------------------------------------------------------------------ forward: one case per reachable instantiation
# (N, Cin, Cout, H, W, k, stride, form).  Ragged in both directions wherever the form allows it: the pixel count is not a multiple of
# the tile's pixel columns, and the last channel tile is partly empty.
FWD_CASES = [
    # big 256 x 256: 3 x 3 over > 256 channels (no short loop) with launch efficiency >= 0.70; the 1 x 1 over 512 channels
    (64, 320, 448, 29, 17, 3, 1, BIG256),       # 123.25 pixel tiles, 448 of 512 channel rows
    (181, 512, 496, 19, 19, 1, 1, BIG256),      # two rounds of 256 tiles, ragged both ways
    # big 128 x 512: 96 < Cout <= 128
    (40, 320, 120, 61, 53, 3, 1, BIG128),       # 252.6 pixel tiles, 120 of 128 rows
    # deep pipeline: >= 16 k32 steps, <= 512 64-channel workgroups, Cout <= 64 or a multiple of 64
    (2, 320, 256, 19, 19, 3, 1, DEEP),
    (2, 640, 64, 9, 9, 3, 1, DEEP),
    (2, 320, 40, 19, 19, 3, 1, DEEP),           # 40 of 64 channel rows
    # short loop: taps x Cin <= 1152
    (3, 64, 24, 13, 11, 3, 1, SHORT32),
    (3, 64, 56, 13, 11, 3, 1, SHORT64),
    (3, 64, 136, 13, 11, 3, 1, SHORT128),
    (3, 128, 200, 13, 11, 1, 1, SHORT128),      # the 1 x 1 rule (<= 128 channels)
    # classic, k16 steps (Cin % 32 != 0)
    (2, 48, 40, 9, 7, 3, 1, classic(1, 2, 2, 2, 16)),
    (2, 48, 88, 9, 7, 3, 1, classic(3, 1, 1, 4, 16)),
    (2, 48, 188, 9, 7, 3, 1, classic(3, 2, 2, 2, 16)),
    (2, 48, 200, 9, 7, 3, 1, classic(2, 2, 2, 2, 16)),
    (2, 48, 256, 9, 7, 3, 1, classic(1, 2, 2, 2, 16)),   # the fill rule: few 128-channel tiles -> 64-channel tiles
    # classic, k32 steps: Cout % 8 != 0 (unstaged stores) ...
    (3, 96, 60, 11, 9, 3, 1, classic(1, 2, 2, 2, 32)),
    (3, 96, 92, 11, 9, 3, 1, classic(3, 1, 1, 4, 32)),
    (3, 96, 100, 11, 9, 3, 1, classic(2, 2, 2, 2, 32)),
    (3, 96, 188, 11, 9, 3, 1, classic(3, 2, 2, 2, 32)),
    # ... and staged (taps x Cin in (1152, 2304] on a small launch: no short loop; Cin % 64 != 0: no deep loop)
    (2, 160, 56, 9, 7, 3, 1, classic(1, 2, 2, 2, 32)),
    (2, 160, 88, 9, 7, 3, 1, classic(3, 1, 1, 4, 32)),
    (2, 160, 120, 9, 7, 3, 1, classic(2, 2, 2, 2, 32)),
    (2, 160, 184, 9, 7, 3, 1, classic(3, 2, 2, 2, 32)),
    # classic, k64 steps: Cout % 8 != 0 ...
    (2, 192, 60, 7, 7, 3, 1, classic(1, 2, 2, 2, 64)),
    (2, 192, 92, 7, 7, 3, 1, classic(3, 1, 1, 4, 64)),
    (2, 192, 100, 7, 7, 3, 1, classic(2, 2, 2, 2, 64)),
    (2, 192, 188, 7, 7, 3, 1, classic(3, 2, 2, 2, 64)),
    # ... and staged: launches neither the big, the short nor the deep form takes
    (4, 1088, 64, 129, 129, 1, 1, classic(1, 2, 2, 2, 64)),   # 521 64-channel workgroups: too many for the deep loop
    (2, 320, 88, 9, 7, 3, 1, classic(3, 1, 1, 4, 64)),
    (2, 512, 200, 13, 13, 1, 1, classic(2, 2, 2, 2, 64)),
    (2, 512, 568, 13, 13, 1, 1, classic(3, 2, 2, 2, 64)),
    # stride 2 (istep 2: the decoded, non-linear source addressing)
    (2, 64, 56, 13, 11, 3, 2, SHORT64),
    (2, 320, 256, 19, 19, 3, 2, DEEP),
    (2, 48, 88, 13, 11, 3, 2, classic(3, 1, 1, 4, 16)),
]


def _fid(c):
    return "N%d_%d-%d_%dx%d_k%d_s%d_%s" % (c[:7] + ("-".join(str(int(v)) for v in c[7][:5]) + ("_fp8" if c[7][5] else "") +
                                                   ("_ns%d" % c[7][6] if c[7][6] != 2 else "") + ("_mb%d" % c[7][7] if c[7][7] != 2 else ""),))


# (act, residual mode) combinations of the epilogue sweep: every activation code with no residual, the residual before and after it
EPILOGUES = [(a, r) for a in range(7) for r in ("none", "before", "after")]
# the cases that also run the whole sweep: one per form family and store path
SWEEP = {(64, 320, 448, 29, 17, 3, 1), (40, 320, 120, 61, 53, 3, 1), (2, 320, 40, 19, 19, 3, 1), (3, 64, 24, 13, 11, 3, 1),
         (3, 64, 56, 13, 11, 3, 1), (3, 64, 136, 13, 11, 3, 1), (2, 48, 188, 9, 7, 3, 1), (3, 96, 92, 11, 9, 3, 1),
         (2, 160, 184, 9, 7, 3, 1), (2, 512, 568, 13, 13, 1, 1), (2, 64, 56, 13, 11, 3, 2)}


@pytest.mark.parametrize("case", FWD_CASES, ids=[_fid(c) for c in FWD_CASES])
def test_gather_form_forward(case):
    """forward + statistics + bias on the form the case names; the swept cases then run every activation code with and without a
    residual (before / after the activation), alternately with the inference epilogue (ch_scale + bias)"""
    from holocron_amd import _lib
    from holocron_amd.ops import conv as cv
    N, Cin, Cout, H, W, k, stride, form = case
    pad = k // 2
    g, x, w = operands(N, Cin, Cout, H, W, k, 1)
    acc, A = fwd_ref(x, w, stride, pad)
    OH, OW = acc.shape[2], acc.shape[3]
    bc, bp = tile(form)
    if (N * OH * OW) % bp == 0 and Cout % bc == 0:
        pytest.fail("case is not ragged in either direction: %s" % (case,))
    bias = torch.randn((Cout,), generator=g)
    xg, wpk, bg = cv.to_cl_bf16(x.to(DEV)), cv.pack_weight(w.to(DEV), 0), bias.to(DEV)
    out = Guarded(N, Cout, OH, OW)
    d = cv.fwd_desc(N, Cin, H, W, Cout, k, k, stride, pad)
    stats = torch.zeros((_lib.stat_replicas(), 2, Cout), device=DEV)
    got_form = launch(d, xg, wpk, out.t, stats=stats, bias=bg)
    assert got_form == form, (case, got_form)
    got = out.check(case)
    ref = acc + bias.view(1, -1, 1, 1)
    check_bound(got, ref, A, case)
    assert rel_l2(got, ref) < 3e-3
    check_stats(stats, acc, case)
    if case[:7] not in SWEEP:
        return
    resid = bf16r(torch.randn((N, Cout, OH, OW), generator=g))
    rg = cv.to_cl_bf16(resid.to(DEV))
    cs = torch.rand((Cout,), generator=g) * 1.5 + 0.25
    cs[::3] *= -1
    csg = cs.to(DEV)
    for i, (act, rmode) in enumerate(EPILOGUES):
        use_cs = (act + i) % 2 == 1
        slope = 0.2 if act == 3 else 0.0
        out.reset()
        f = launch(d, xg, wpk, out.t, bias=bg, act=act, resid=None if rmode == "none" else rg, ch_scale=csg if use_cs else None,
                   act_slope=slope, resid_after_act=rmode == "after")
        what = (case, act, rmode, "ch_scale" if use_cs else "bias")
        assert f == form, (what, f)
        got = out.check(what)
        v = acc * (cs.view(1, -1, 1, 1) if use_cs else 1.0) + bias.view(1, -1, 1, 1)
        Ae = A * (cs.abs().view(1, -1, 1, 1) if use_cs else 1.0)
        if rmode == "before":
            v = v + resid
        v = act_ref(v, act, slope if act == 3 else 0.1)
        if rmode == "after":
            v = v + resid
        Ae = Ae * (1.25 if act else 1.0) + (resid.abs() if rmode != "none" else 0.0)
        check_bound(got, v, Ae, what)


# ------------------------------------------------------------------ fp8 inference forms (ch_mult set, through the descriptor)
def _fp8r(t):
    return t.clamp(-448, 448).to(torch.float8_e4m3fn).float()


FP8_CASES = [(64, fp8form(1, 2, 2, 2)), (60, fp8form(1, 2, 2, 2)), (96, fp8form(3, 1, 1, 4)), (68, fp8form(3, 1, 1, 4)),
             (192, fp8form(3, 2, 2, 2)), (128, fp8form(2, 2, 2, 2))]


@pytest.mark.parametrize("Cout,form", FP8_CASES, ids=["cout%d" % c for c, _ in FP8_CASES])
def test_gather_form_fp8(Cout, form):
    """fp8 bytes through hc_conv_gather (ch_mult) at a Cout the C ABI accepts (% 4 == 0, not padded to 64) and a ragged pixel count,
    against fp32 math on the same fp8 values: equal except for requantisation flips at fp8 rounding boundaries"""
    from holocron_amd import _lib
    from holocron_amd.ops import conv as cv
    from holocron_amd.models.classification.repvgg_fp8 import quantize_weight_fp8
    N, Cin, H, W, k, stride, pad = 2, 64, 9, 7, 3, 1, 1
    g = gen(8, Cout)
    x = _fp8r(torch.randn((N, Cin, H, W), generator=g) * 2)
    w = torch.randn((Cout, Cin, k, k), generator=g) * 0.1
    bias = torch.randn((Cout,), generator=g)
    sx_in, sx_out = 0.5, 0.25
    sw = w.abs().amax(dim=(1, 2, 3)) / 448
    wq = _fp8r(w / sw.view(-1, 1, 1, 1))
    acc = F.conv2d(x, wq, None, stride, pad)
    ref = _fp8r(torch.relu(acc * (sw * sx_in / sx_out).view(1, -1, 1, 1) + (bias / sx_out).view(1, -1, 1, 1)))
    wpk, swp = quantize_weight_fp8(w.to(DEV), Cin, Cout)
    xq = x.permute(0, 2, 3, 1).contiguous().to(torch.float8_e4m3fn).view(torch.uint8).to(DEV)
    d = cv.fwd_desc(N, Cin, H, W, Cout, k, k, stride, pad)
    out = Guarded(N, Cout, d.OH, d.OW, fp8=True)
    mult = (swp * (sx_in / sx_out)).contiguous()
    d.ch_mult = _lib.ptr(mult)
    f = launch(d, xq, wpk, out.t, bias=(bias / sx_out).to(DEV), act=1)
    assert f == form, (Cout, f)
    got = out.check(("fp8", Cout)).view(torch.float8_e4m3fn).float()
    same = float((got == ref).float().mean())
    assert same > 0.99, (Cout, same)
    assert float(((got - ref).abs() <= 0.126 * ref.abs().clamp(min=2 ** -6)).float().mean()) == 1.0


# ------------------------------------------------------------------ epilogue features the classic form alone takes
SCALAR_CASES = [(30, classic(1, 2, 2, 2, 64)), (90, classic(3, 1, 1, 4, 64)), (250, classic(2, 2, 2, 2, 64)),
                (190, classic(3, 2, 2, 2, 64))]


@pytest.mark.parametrize("Cout,form", SCALAR_CASES, ids=["cout%d" % c for c, _ in SCALAR_CASES])
def test_gather_scalar_stores(Cout, form):
    """Cout % 4 != 0: the per-element store path, with statistics, residual before / after the activation and ch_scale"""
    from holocron_amd import _lib
    from holocron_amd.ops import conv as cv
    N, Cin, H, W = 2, 192, 7, 9
    g, x, w = operands(N, Cin, Cout, H, W, 3, 3)
    acc, A = fwd_ref(x, w, 1, 1)
    bias = torch.randn((Cout,), generator=g)
    resid = bf16r(torch.randn(acc.shape, generator=g))
    cs = torch.rand((Cout,), generator=g) + 0.5
    xg, wpk = cv.to_cl_bf16(x.to(DEV)), cv.pack_weight(w.to(DEV), 0)
    out = Guarded(N, Cout, H, W)
    d = cv.fwd_desc(N, Cin, H, W, Cout, 3, 3, 1, 1)
    for act, rmode, use_cs in ((0, "none", False), (5, "before", False), (3, "after", True), (4, "before", True)):
        stats = torch.zeros((_lib.stat_replicas(), 2, Cout), device=DEV)
        out.reset()
        f = launch(d, xg, wpk, out.t, stats=stats, bias=bias.to(DEV), act=act, resid=None if rmode == "none" else cv.to_cl_bf16(resid.to(DEV)),
                   ch_scale=cs.to(DEV) if use_cs else None, act_slope=0.3 if act == 3 else 0.0, resid_after_act=rmode == "after")
        what = (Cout, act, rmode, use_cs)
        assert f == form, (what, f)
        got = out.check(what)
        v = acc * (cs.view(1, -1, 1, 1) if use_cs else 1.0) + bias.view(1, -1, 1, 1)
        if rmode == "before":
            v = v + resid
        v = act_ref(v, act, 0.3)
        if rmode == "after":
            v = v + resid
        Ae = A * (cs.view(1, -1, 1, 1) if use_cs else 1.0) * 1.25 + (resid.abs() if rmode != "none" else 0.0)
        check_bound(got, v, Ae, what)
        check_stats(stats, acc, what)


CO_SPLIT_CASES = [(20, 44, classic(1, 2, 2, 2, 64)), (32, 56, classic(3, 1, 1, 4, 64)), (64, 124, classic(3, 2, 2, 2, 64))]


@pytest.mark.parametrize("C1,C2,form", CO_SPLIT_CASES, ids=["%d+%d" % c[:2] for c in CO_SPLIT_CASES])
def test_gather_co_split(C1, C2, form):
    """two stacked convolutions of one source (co_split): two destinations with their own channel counts and two sets of statistics;
    a split that is not a multiple of 8 and a total that is not takes the unstaged stores"""
    from holocron_amd import _lib
    from holocron_amd.ops import conv as cv
    N, Cin, H, W = 3, 64, 9, 7
    g, x, w = operands(N, Cin, C1 + C2, H, W, 3, 4)
    acc, A = fwd_ref(x, w, 1, 1)
    xg, wpk = cv.to_cl_bf16(x.to(DEV)), cv.pack_weight(w.to(DEV), 0)
    o1, o2 = Guarded(N, C1, H, W), Guarded(N, C2, H, W)
    s1 = torch.zeros((_lib.stat_replicas(), 2, C1), device=DEV)
    s2 = torch.zeros((_lib.stat_replicas(), 2, C2), device=DEV)
    d = cv.fwd_desc(N, Cin, H, W, C1 + C2, 3, 3, 1, 1)
    f = launch(d, xg, wpk, o1.t, stats=s1, dst2=o2.t, stats2=s2, co_split=C1)
    assert f == form, ((C1, C2), f)
    for o, sl, st in ((o1, slice(0, C1), s1), (o2, slice(C1, C1 + C2), s2)):
        got = o.check((C1, C2, sl))
        check_bound(got, acc[:, sl], A[:, sl], (C1, C2, sl))
        check_stats(st, acc[:, sl], (C1, C2, sl))


NORM_CASES = [(2, 64, 96, 9, 7, classic(3, 1, 1, 4, 64)), (2, 48, 40, 11, 9, classic(1, 2, 2, 2, 16)),
              (3, 96, 184, 7, 7, classic(3, 2, 2, 2, 32))]


@pytest.mark.parametrize("N,Cin,Cout,H,W,form", NORM_CASES, ids=["%d-%d" % c[1:3] for c in NORM_CASES])
def test_gather_pix_scale(N, Cin, Cout, H, W, form):
    """NormConv2d epilogue: v = pix_scale[p] * (acc - pix_shift[p] * ch_coef[co]) + bias, then the activation"""
    from holocron_amd.ops import conv as cv
    g, x, w = operands(N, Cin, Cout, H, W, 3, 5)
    acc, A = fwd_ref(x, w, 1, 1)
    bias = torch.randn((Cout,), generator=g)
    ps = torch.rand((N, H, W), generator=g) + 0.5
    pm = torch.randn((N, H, W), generator=g)
    coef = torch.randn((Cout,), generator=g)
    psg, pmg, cg = ps.to(DEV).contiguous(), pm.to(DEV).contiguous(), coef.to(DEV)
    xg, wpk = cv.to_cl_bf16(x.to(DEV)), cv.pack_weight(w.to(DEV), 0)
    out = Guarded(N, Cout, H, W)
    d = cv.fwd_desc(N, Cin, H, W, Cout, 3, 3, 1, 1)
    d.pix_scale, d.pix_shift, d.ch_coef = psg.data_ptr(), pmg.data_ptr(), cg.data_ptr()
    f = launch(d, xg, wpk, out.t, bias=bias.to(DEV), act=1)
    assert f == form, f
    got = out.check("pix_scale")
    p4, m4 = ps.view(N, 1, H, W), pm.view(N, 1, H, W)
    ref = F.relu(p4 * (acc - m4 * coef.view(1, -1, 1, 1)) + bias.view(1, -1, 1, 1))
    Ae = p4 * (A + (m4 * coef.view(1, -1, 1, 1)).abs())
    check_bound(got, ref, Ae, "pix_scale")


# ------------------------------------------------------------------ stride-2 data gradients (four parity classes of unequal size)
def _dgrad(N, Cin, Cout, H, W, dual, seed):
    """dx of conv3x3(x, stride 2, pad 1) [+ conv1x1(x, stride 2)] wrt x, + resid: operands, reference and the descriptor"""
    from holocron_amd.ops import conv as cv
    g = gen(seed, N, Cin, Cout, H, W, int(dual))
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    w3 = bf16r(torch.randn((Cout, Cin, 3, 3), generator=g) / (Cout * 9) ** 0.5)
    dy3 = bf16r(torch.randn((N, Cout, OH, OW), generator=g))
    resid = bf16r(torch.randn((N, Cin, H, W), generator=g))
    ref = conv2d_input((N, Cin, H, W), w3, dy3, 2, 1) + resid
    A = conv2d_input((N, Cin, H, W), w3.abs(), dy3.abs(), 2, 1) + resid.abs()
    branches, T = [(3, 3, 1, 0, 0)], 9
    w1 = dy1 = None
    if dual:
        w1 = bf16r(torch.randn((Cout, Cin, 1, 1), generator=g) / Cout ** 0.5)
        dy1 = bf16r(torch.randn((N, Cout, OH, OW), generator=g))
        ref = ref + conv2d_input((N, Cin, H, W), w1, dy1, 2, 0)
        A = A + conv2d_input((N, Cin, H, W), w1.abs(), dy1.abs(), 2, 0)
        branches, T = branches + [(1, 1, 0, 1, 9)], 10
    d = cv.dgrad_desc(N, Cin, H, W, Cout, branches, 2)
    wp = torch.empty((Cin, T, Cout), dtype=torch.bfloat16, device=DEV)
    cv.pack_weight(w3.to(DEV), 1, out=wp, tap0=0, T=T)
    if dual:
        cv.pack_weight(w1.to(DEV), 1, out=wp, tap0=9, T=T)
    return d, wp, dy3, dy1, resid, ref, A


DGRAD_CASES = [
    # N, Cin (dx channels), Cout (dy channels), H, W (odd: class grids 7/6 x 6/5), dual, form
    (2, 56, 64, 13, 11, False, SHORT64),
    (2, 56, 64, 13, 11, True, SHORT64),
    (2, 64, 512, 13, 11, False, DEEP),          # the 1-tap class has 16 k32 steps
    (2, 40, 320, 13, 11, True, DEEP),           # the 2-tap classes: 20 k32 steps; 40 of 64 channel rows
    (2, 40, 48, 13, 11, False, classic(1, 2, 2, 2, 16)),
    (2, 88, 48, 13, 11, True, classic(3, 1, 1, 4, 16)),
]


@pytest.mark.parametrize("N,Cin,Cout,H,W,dual,form", DGRAD_CASES, ids=["%d-%d_%dx%d_%s" % (c[1], c[2], c[3], c[4], "dual" if c[5] else "single")
                                                                     for c in DGRAD_CASES])
def test_gather_dgrad_stride2(N, Cin, Cout, H, W, dual, form):
    from holocron_amd.ops import conv as cv
    d, wp, dy3, dy1, resid, ref, A = _dgrad(N, Cin, Cout, H, W, dual, 6)
    out = Guarded(N, Cin, H, W)
    f = launch(d, cv.to_cl_bf16(dy3.to(DEV)), wp, out.t, src1=None if dy1 is None else cv.to_cl_bf16(dy1.to(DEV)),
               resid=cv.to_cl_bf16(resid.to(DEV)))
    assert f == form, f
    got = out.check("dgrad")
    check_bound(got, ref, A, ("dgrad", Cin, Cout, dual))
    assert rel_l2(got, ref) < 3e-3


def _dgrad_rows_ref(dy, w, a, b, W):
    """rows [2a + 1, 2b - 2] of conv2d_input(stride 2, pad 1, 3 x 3) of ONE image from the dy rows [a, b) alone"""
    Hc = 2 * (b - a) - 1
    full = conv2d_input((1, w.shape[1], Hc, W), w, dy[:, :, a:b], 2, 1)
    return full[:, :, 1:Hc - 1]


def test_gather_dgrad_class_fastest_order():
    """a stride-2 data gradient whose dy is >= 128 MB: the parity classes become the fastest index of the tile order (flags bit 1);
    all of dx is checked for NaN / guards, sampled images against the CPU"""
    from holocron_amd.ops import conv as cv
    N, Cin, Cout, H, W = 8, 32, 64, 735, 735
    OH = (H - 1) // 2 + 1
    assert N * OH * OH * Cout * 2 >= 128e6
    g = gen(9)
    w = bf16r(torch.randn((Cout, Cin, 3, 3), generator=g) / (Cout * 9) ** 0.5)
    dyg = torch.empty((N, OH, OH, Cout), dtype=torch.bfloat16, device=DEV)
    dyg.normal_(generator=torch.Generator(device=DEV).manual_seed(9))
    dyg = dyg.permute(0, 3, 1, 2)
    wp = cv.pack_weight(w.to(DEV), 1)
    d = cv.dgrad_desc(N, Cin, H, W, Cout, [(3, 3, 1, 0, 0)], 2)
    out = Guarded(N, Cin, H, W)
    f = launch(d, dyg, wp, out.t)
    assert f == SHORT32, f
    got = out.check("class-fastest dgrad")
    for n in (0, N - 1):
        dy = dyg[n:n + 1].float().cpu()
        ref, A = conv2d_input((1, Cin, H, W), w, dy, 2, 1), conv2d_input((1, Cin, H, W), w.abs(), dy.abs(), 2, 1)
        check_bound(got[n:n + 1], ref, A, ("class-fastest dgrad", n))
    del out, dyg


# ------------------------------------------------------------------ the top of the 32-bit source range
def _rows_fwd_ref(x, w, r0, r1):
    """rows [r0, r1) of conv2d(x, w, stride 1, pad 1) of one image (x: [1][C][H][W] CPU) from the x rows they need"""
    H = x.shape[2]
    lo, hi = max(r0 - 1, 0), min(r1 + 1, H)
    xc = F.pad(x[:, :, lo:hi], (1, 1, 1 if r0 == 0 else 0, 1 if r1 == H else 0))
    return F.conv2d(xc, w), F.conv2d(xc.abs(), w.abs())


def test_gather_forward_source_above_2gib():
    """3 x 3 pad 1 on a bf16 source of 2.22 GB (> 2^31 bytes, < the 4 GiB limit of the unsigned buffer offsets): the last image whole,
    row bands of earlier images (the first rows, the middle of the tensor, the rows just below 2^31 bytes)"""
    from holocron_amd import _lib
    from holocron_amd.ops import conv as cv
    N, Cin, Cout, H, W = 32, 64, 32, 736, 736
    assert 2 ** 31 < N * H * W * Cin * 2 < 4294967280
    g = gen(10)
    w = bf16r(torch.randn((Cout, Cin, 3, 3), generator=g) / (Cin * 9) ** 0.5)
    xg = torch.empty((N, H, W, Cin), dtype=torch.bfloat16, device=DEV)
    xg.normal_(generator=torch.Generator(device=DEV).manual_seed(10))
    xg = xg.permute(0, 3, 1, 2)
    d = cv.fwd_desc(N, Cin, H, W, Cout, 3, 3, 1, 1)
    out = Guarded(N, Cout, H, W)
    stats = torch.zeros((_lib.stat_replicas(), 2, Cout), device=DEV)
    f = launch(d, xg, cv.pack_weight(w.to(DEV), 0), out.t, stats=stats)
    assert f == SHORT32, f
    got = out.check("2 GiB forward")
    per_img = H * W * Cin * 2
    n31 = (2 ** 31) // per_img                     # the image that straddles 2^31 bytes
    r31 = ((2 ** 31) % per_img) // (W * Cin * 2)
    for n, r0, r1 in ((N - 1, 0, H), (0, 0, 8), (N // 2, 360, 376), (n31, max(r31 - 8, 0), min(r31 + 8, H)), (N - 2, H - 8, H)):
        x = xg[n:n + 1].float().cpu()
        ref, A = _rows_fwd_ref(x, w, r0, r1)
        check_bound(got[n:n + 1, :, r0:r1], ref, A, ("2 GiB forward", n, r0))
    del out, xg


def test_gather_dgrad_source_above_2gib():
    """stride-2 data gradient whose dy is 2.22 GB: the last image whole, row bands of earlier ones"""
    from holocron_amd.ops import conv as cv
    N, Cin, Cout, H, W = 32, 32, 64, 1471, 1471
    OH = (H - 1) // 2 + 1
    assert 2 ** 31 < N * OH * OH * Cout * 2 < 4294967280
    g = gen(11)
    w = bf16r(torch.randn((Cout, Cin, 3, 3), generator=g) / (Cout * 9) ** 0.5)
    dyg = torch.empty((N, OH, OH, Cout), dtype=torch.bfloat16, device=DEV)
    dyg.normal_(generator=torch.Generator(device=DEV).manual_seed(11))
    dyg = dyg.permute(0, 3, 1, 2)
    d = cv.dgrad_desc(N, Cin, H, W, Cout, [(3, 3, 1, 0, 0)], 2)
    out = Guarded(N, Cin, H, W)
    f = launch(d, dyg, cv.pack_weight(w.to(DEV), 1), out.t)
    assert f == SHORT32, f
    got = out.check("2 GiB dgrad")
    n = N - 1
    dy = dyg[n:n + 1].float().cpu()
    check_bound(got[n:n + 1], conv2d_input((1, Cin, H, W), w, dy, 2, 1), conv2d_input((1, Cin, H, W), w.abs(), dy.abs(), 2, 1),
                ("2 GiB dgrad", n))
    for n, a in ((0, 0), (N // 2, 300), (N - 2, OH - 12)):
        dy = dyg[n:n + 1].float().cpu()
        b = a + 12
        ref, A = _dgrad_rows_ref(dy, w, a, b, W), _dgrad_rows_ref(dy.abs(), w.abs(), a, b, W)
        check_bound(got[n:n + 1, :, 2 * a + 1:2 * b - 2], ref, A, ("2 GiB dgrad", n, a))
    del out, dyg


# ------------------------------------------------------------------ deterministic mode
@pytest.mark.parametrize("shape,form", [((64, 320, 448, 29, 17), BIG256), ((2, 320, 256, 19, 19), DEEP)], ids=["big", "deep"])
def test_gather_deterministic_statistics(shape, form):
    """hc_set_deterministic(1): every workgroup owns a statistics replica, two launches give bit-identical sums"""
    from holocron_amd import _lib
    from holocron_amd.ops import conv as cv
    N, Cin, Cout, H, W = shape
    g, x, w = operands(N, Cin, Cout, H, W, 3, 12)
    xg, wpk = cv.to_cl_bf16(x.to(DEV)), cv.pack_weight(w.to(DEV), 0)
    d = cv.fwd_desc(N, Cin, H, W, Cout, 3, 3, 1, 1)
    out = Guarded(N, Cout, H, W)
    _lib.set_deterministic(True)
    try:
        runs = []
        for _ in range(2):
            stats = torch.zeros((_lib.stat_replicas(), 2, Cout), device=DEV)
            out.reset()
            f = launch(d, xg, wpk, out.t, stats=stats)
            assert f == form, f
            runs.append(stats)
        assert torch.equal(runs[0], runs[1])
        got = out.check("deterministic")
    finally:
        _lib.set_deterministic(False)
    acc, A = fwd_ref(x, w, 1, 1)
    check_bound(got, acc, A, "deterministic")
    check_stats(runs[0], acc, "deterministic")


def test_gather_deterministic_refuses_too_many_pixel_tiles():
    """with statistics, a grid of more pixel tiles than hc_get_stat_replicas() is refused (HC_ERR_ARG), not run"""
    from holocron_amd import _lib
    from holocron_amd._lib import ptr, stream
    from holocron_amd.ops import conv as cv
    N, Cin, Cout, H, W = 17, 32, 64, 500, 500        # short form, 128-pixel tiles: 33 204 of them
    lib = _lib.load()
    x = cv.empty_cl(N, Cin, H, W, DEV).zero_()
    y = cv.empty_cl(N, Cout, H, W, DEV)
    wpk = torch.zeros((Cout, 9, Cin), dtype=torch.bfloat16, device=DEV)
    d = cv.fwd_desc(N, Cin, H, W, Cout, 3, 3, 1, 1)
    _lib.set_deterministic(True)
    try:
        reps = _lib.stat_replicas()
        assert (N * H * W + 127) // 128 > reps
        stats = torch.zeros((reps, 2, Cout), device=DEV)
        d.src0, d.wpk, d.dst, d.stats = ptr(x), ptr(wpk), ptr(y), ptr(stats)
        rc = lib.hc_conv_gather(C.byref(d), stream())
        torch.cuda.synchronize()
        assert rc == 1, rc
        assert float(stats.abs().sum()) == 0.0
    finally:
        _lib.set_deterministic(False)
