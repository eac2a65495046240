"""Per-layer parity at the BASELINE sizes: every distinct block shape of repvgg_a0 at batch 256 (BASELINE.json configs[1],
SURVEY.md §8d table), the distinct YOLOv4 conv shapes at 608 x 608 / batch 16 (configs[3]) and the ReXNet
depthwise / pointwise shapes at batch 256 (configs[2]) - HIP kernels against torch-CPU fp32 (`F.conv2d` + the closed-form
gradients `torch.nn.grad.conv2d_input / conv2d_weight`) on identical bf16-representable operands.

These are the launch geometries that only exist at full size (112 tiles per persistent workgroup in the small-channel conv,
the many-way split-K weight gradients, the DMA kernels on 1280 channels, XCD-grouped tile orders).  Layers are compared in
ISOLATION: one block of a randomly initialised network has no chaotic amplification, so the bounds are the rounding of the
stored dtype and nothing else:

* bf16-stored outputs (conv results, data gradients): rel-L2 <= 2e-3.  One round-to-nearest-even to bf16 (8 significant bits)
  is off by up to half an ulp = 2^-8 / m of the element (m in [1, 2) its significand) -> RMS 2^-8 / sqrt(3) * sqrt(E[1/m^2]) =
  1.6e-3 (measured on the MI355X: 1.64-1.66e-3 on every shape): north_star's 1e-3 is below what ONE bf16 store of an exact
  result can meet.  The data gradient of an identity block adds the identity-branch gradient to the bf16-staged conv result
  and rounds again (csrc/conv_small.hip `store`): two roundings, 1.65e-3 * sqrt(2) = 2.3e-3 measured, bound 2.6e-3.
* fp32 outputs (weight gradients, BatchNorm statistics and parameter gradients): rel-L2 <= 2e-4 (fp32 accumulation order).
* a whole RepBlock forward / backward against the bf16-EMULATING oracle (oracle.repvgg.rep_block_bf16: the reference's
  arithmetic with a bf16 rounding exactly where the HIP path stores bf16, forward AND backward): <= 5e-4 on `out`, 1e-3 on dx
  and the conv weight gradients (isolated 1-ulp flips), 2e-4 on the BatchNorm parameter gradients; against the plain fp32
  reference block: out <= 4e-3 (three stored roundings: y3, y1, out), gradients reported (see the comment in the test).

The batch can be lowered with HC_FULLSIZE_N for a quick run; the default is the BASELINE size.
"""
import os

import pytest
import torch
import torch.nn.functional as F

from conftest import rel_l2

pytestmark = pytest.mark.gpu

N_C2 = int(os.environ.get("HC_FULLSIZE_N", "256"))
N_C4 = int(os.environ.get("HC_FULLSIZE_N_YOLO", "16"))
TOL_BF16 = 2e-3
TOL_F32 = 2e-4


def bf16r(t):
    return t.to(torch.bfloat16).to(torch.float32)


def nchw(t):
    return t.float().cpu().contiguous()


def gen(seed):
    return torch.Generator().manual_seed(seed)


def stem_fused_on():
    from holocron_amd import _lib
    import ctypes as C
    d = _lib.StemDesc()
    d.N, d.H, d.W = 1, 224, 224
    return bool(_lib.load().hc_stem_fused_supported(C.byref(d)))


# (Cin, Cout, H, stride, identity): the ten rows of SURVEY.md §8d (repvgg_a0, 224 x 224 input)
C2_BLOCKS = [
    (3, 48, 224, 2, False),
    (48, 48, 112, 1, True),
    (48, 48, 112, 2, False),
    (48, 48, 56, 1, True),
    (48, 96, 56, 2, False),
    (96, 96, 28, 1, True),
    (96, 192, 28, 2, False),
    (192, 192, 14, 1, True),
    (192, 1280, 14, 2, False),
    (1280, 1280, 7, 1, True),
]
C2_IDS = ["%d@%d-%d_s%d" % (c[0], c[2], c[1], c[3]) for c in C2_BLOCKS]


def _stat_check(stats, ref, what):
    """stats [R][2][C] replicas of sum / sum of squares vs the fp32 conv result `ref` (NCHW)."""
    s = stats.double().sum(0).cpu()
    r = ref.double()
    cnt = r.numel() / r.shape[1]
    s1, s2 = r.sum((0, 2, 3)), (r * r).sum((0, 2, 3))
    # a sum of signed values cancels: bound its error against the magnitude the accumulation carries
    scale1 = torch.sqrt(s2 * cnt) + 1e-30
    assert float(((s[0] - s1).abs() / scale1).max()) < TOL_F32, (what, "sum")
    assert rel_l2(s[1], s2) < TOL_F32, (what, "sumsq")


@pytest.mark.parametrize("cfg", C2_BLOCKS, ids=C2_IDS)
def test_c2_conv_passes_vs_fp32_cpu(cfg):
    """forward 3x3 + 1x1 (with the statistics epilogue), fused data gradient and both weight gradients of one block shape,
    through the same launch helpers RepBlockFn uses (nn/repblock_op.py: block_convs_forward / block_dgrad / block_wgrad).
    Reference ops: aten::convolution / convolution_backward behind nn.Conv2d (models/utils.py:73, repvgg.py:57-60)."""
    _c2_conv_passes(cfg)


@pytest.mark.parametrize("cfg", C2_BLOCKS, ids=C2_IDS)
def test_c2_conv_passes_deterministic_mode_vs_fp32_cpu(cfg):
    """The same passes under ``set_deterministic(True)``: single-writer statistics slots (32768 replicas, per-wave LDS planes in
    a fixed order instead of `ds_add_f32`) and single-writer split reductions are DIFFERENT code paths in every conv kernel;
    round 2 only compared them with themselves (bit-identical reruns).  Here: against torch-CPU fp32, same bounds."""
    import holocron_amd as h
    h.set_deterministic(True)
    try:
        _c2_conv_passes(cfg)
    finally:
        h.set_deterministic(False)


# Block shapes of the OTHER RepVGG variants (repvgg.py:146-154, 224 x 224 input): repvgg_a1 / b0 (64, 128, 256 channels) and
# repvgg_a2 (96, 192, 384) - none of them is a shape a specialised kernel was written for, so this is the generic dispatch
# (gather-conv incl. its big-tile family, image-resident conv, fused / transposing weight gradients) at full map size, batch 64
RV_OTHER_BLOCKS = [
    (64, 64, 56, 1, True), (128, 128, 28, 1, True), (256, 256, 14, 1, True), (128, 256, 28, 2, False),
    (96, 96, 56, 1, True), (192, 192, 28, 1, True), (384, 384, 14, 1, True), (192, 384, 28, 2, False),
]


@pytest.mark.parametrize("cfg", RV_OTHER_BLOCKS, ids=["%d@%d-%d_s%d" % (c[0], c[2], c[1], c[3]) for c in RV_OTHER_BLOCKS])
def test_other_repvgg_block_shapes_vs_fp32_cpu(cfg):
    """The same four passes (forward 3x3 + 1x1 + statistics, fused data gradient, both weight gradients) as test_c2_conv_passes_* for
    the block shapes of repvgg_a1 / b0 / a2, against torch-CPU fp32 convolutions, same bounds."""
    _c2_conv_passes(cfg, N=64)


def _c2_conv_passes(cfg, N=None):
    from holocron_amd import _lib
    from holocron_amd.nn import repblock_op as rb
    from holocron_amd.ops import conv as cv
    cin, cout, H, stride, ident = cfg
    N = N_C2 if N is None else N
    g = gen(1000 + cin + cout + H)
    x = bf16r(torch.rand((N, cin, H, H), generator=g))
    w3 = bf16r(torch.randn((cout, cin, 3, 3), generator=g) * (2.0 / (cout * 9)) ** 0.5)
    w1 = bf16r(torch.randn((cout, cin, 1, 1), generator=g) * (2.0 / cout) ** 0.5)
    dev = torch.device("cuda:0")
    st = rb.RepState(stride, ident)
    stem = cin % 16 != 0
    xg = x.to(dev)
    src = cv.im2col_small(xg, 3, 3, stride, 1, rb.STEM_KPAD) if stem else cv.to_cl_bf16(xg)
    w3g, w1g = w3.to(dev), w1.to(dev)
    geom = (N, cin, H, H, cout)
    stats = torch.zeros((2, _lib.stat_replicas(), 2, cout), device=dev)
    # the stem's forward reads the image batch itself when the stride-2 row kernel takes it (no column tensor; csrc/conv_s2.hip)
    fsrc = xg if (stem and st.s2_desc(*geom) is not None) else src
    y3, y1 = rb.block_convs_forward(st, fsrc, w3g, w1g, geom, stats, cin if stem else None)
    torch.cuda.synchronize()

    c3 = F.conv2d(x, w3, None, stride, 1)
    c1 = F.conv2d(x, w1, None, stride, 0)
    e3, e1 = rel_l2(nchw(y3), c3), rel_l2(nchw(y1), c1)
    print(f"{cfg}: fwd y3 {e3:.2e} y1 {e1:.2e}")
    assert e3 < TOL_BF16 and e1 < TOL_BF16, (cfg, e3, e1)
    _stat_check(stats[0], c3, (cfg, "3x3"))
    _stat_check(stats[1], c1, (cfg, "1x1"))

    dy3 = bf16r(torch.randn(c3.shape, generator=g))
    dy1 = bf16r(torch.randn(c1.shape, generator=g))
    dy3g, dy1g = cv.to_cl_bf16(dy3.to(dev)), cv.to_cl_bf16(dy1.to(dev))
    del c3, c1, y3, y1
    if not stem:
        res = bf16r(torch.randn(x.shape, generator=g)) if ident else None
        resg = None if res is None else cv.to_cl_bf16(res.to(dev))
        dx = rb.block_dgrad(st, dy3g, dy1g, resg, w3g, w1g, geom)
        torch.cuda.synchronize()
        ref = torch.nn.grad.conv2d_input(x.shape, w3, dy3, stride, 1) + torch.nn.grad.conv2d_input(x.shape, w1, dy1, stride, 0)
        if res is not None:
            ref = ref + res
        ed = rel_l2(nchw(dx), ref)
        print(f"{cfg}: dgrad {ed:.2e}")
        assert ed < (TOL_BF16 if res is None else 1.3 * TOL_BF16), (cfg, ed)
        del ref, dx
    dw3, dw1 = rb.block_wgrad(st, fsrc if stem else src, dy3g, dy1g, w3g, w1g, geom, cin if stem else None)
    torch.cuda.synchronize()
    r3 = torch.nn.grad.conv2d_weight(x, w3.shape, dy3, stride, 1)
    r1 = torch.nn.grad.conv2d_weight(x, w1.shape, dy1, stride, 0)
    ew3, ew1 = rel_l2(dw3.cpu(), r3), rel_l2(dw1.cpu(), r1)
    print(f"{cfg}: wgrad 3x3 {ew3:.2e} 1x1 {ew1:.2e}")
    assert ew3 < TOL_F32 and ew1 < TOL_F32, (cfg, ew3, ew1)


@pytest.mark.parametrize("cfg", C2_BLOCKS, ids=C2_IDS)
def test_c2_block_vs_oracles(cfg):
    """one RepBlock training forward + backward (all BatchNorm passes included) at batch 256 against the bf16-emulating
    oracle (tight) and the plain fp32 reference block (repvgg.py:71-73; three stored roundings)."""
    import holocron_amd as h
    from oracle import repvgg as orv
    cin, cout, H, stride, ident = cfg
    N = N_C2
    g = gen(2000 + cin + cout + H)
    blk = h.models.RepBlock(cin, cout, stride, ident)
    sd = blk.state_dict()
    for k, v in sd.items():
        if v.dim() == 4:
            v.copy_(bf16r(torch.randn(v.shape, generator=g) * (2.0 / (v.shape[0] * v.shape[2] * v.shape[3])) ** 0.5))
        elif k.endswith("weight"):
            v.copy_(torch.rand(v.shape, generator=g) + 0.5)
        elif k.endswith("bias"):
            v.copy_(torch.randn(v.shape, generator=g) * 0.2)
    state = {k: v.clone() for k, v in sd.items()}
    x = bf16r(torch.rand((N, cin, H, H), generator=g))
    blk = blk.cuda().train()
    xg = x.cuda().requires_grad_(cin % 16 == 0)
    out = blk(xg)
    # upstream gradient with a mean (U[0.5, 1.5)): with a zero-mean random one every channel sum of the backward (sum dz,
    # sum dz*yhat, the weight gradients) is a sqrt(N H W)-sized residual of cancellation - two or three ReLU-mask flips per
    # channel then move it by 1e-3, and the BatchNorm centring terms fall below a bf16 ulp of dy - i.e. the
    # comparison would measure the conditioning of the input, not the kernels
    r = bf16r(torch.rand(out.shape, generator=g) + 0.5)
    (out.float() * r.cuda()).sum().backward()
    torch.cuda.synchronize()
    out_h = nchw(out.detach())
    grads_h = {n: p.grad.detach().cpu() for n, p in blk.named_parameters()}
    dx_h = nchw(xg.grad) if xg.grad is not None else None
    after = {k: v.detach().cpu().clone() for k, v in blk.state_dict().items()}
    del out, xg

    def run(fn, **kw):
        osd = {"blk." + k: v.clone() for k, v in state.items()}
        keys = orv.trainable_keys(osd)
        for k in keys:
            osd[k].requires_grad_(True)
        xe = x.clone().requires_grad_(True)
        o = fn(xe, osd, "blk", stride, ident, True, **kw)
        gr = torch.autograd.grad((o * r).sum(), [xe] + [osd[k] for k in keys])
        return o.detach(), gr[0], {k[4:]: v for k, v in zip(keys, gr[1:])}, osd

    # the stride-1 blocks of <= 48 channels run the persistent small-channel kernel, which stages the data gradient in bf16
    # before it adds the identity-branch gradient (one more rounding, modelled by the oracle)
    # only the persistent small-channel kernel stages dx in bf16 before the residual is added (two roundings); the row-unit kernels
    # (weight image flag 4 in the descriptor's mode) add the residual to the fp32 accumulator
    sd = blk._hc.descs(N, cin, H, H, cout)[4]
    staged = ident and cin < 64 and sd is not None and not (sd.mode & 4)
    # the stem at 224 x 224 runs fused with its BatchNorm passes: y3 / y1 are recomputed in fp32, never stored (one rounding less)
    fused_stem = cin == 3 and blk._hc.desc[(N, cin, H, H, cout)][6] is not None and stem_fused_on()
    eo, edx, eg, esd = run(orv.rep_block_bf16, dx_staged=staged, recompute=fused_stem)
    errs = {"out": rel_l2(out_h, eo)}
    mism = float((out_h != eo).double().mean())
    if dx_h is not None:
        errs["dx"] = rel_l2(dx_h, edx)
    for n, gh in grads_h.items():
        errs["d " + n] = rel_l2(gh, eg[n])
    print(f"{cfg} vs bf16 oracle (out differs in {mism:.2e} of the elements): " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    for k, v in after.items():
        ref = esd["blk." + k].detach()
        if "running" in k:
            assert rel_l2(v, ref) < 1e-5, (cfg, k)
        if k.endswith("num_batches_tracked"):
            assert int(v) == int(ref) == 1
    del eo, edx, esd
    fo, fdx, fg, _ = run(orv.rep_block)
    ferrs = {"out": rel_l2(out_h, fo)}
    if dx_h is not None:
        ferrs["dx"] = rel_l2(dx_h, fdx)
    for n, gh in grads_h.items():
        ferrs["d " + n] = rel_l2(gh, fg[n])
    print(f"{cfg} vs fp32 reference: " + ", ".join(f"{k} {v:.2e}" for k, v in ferrs.items()))
    # Kernel-level bounds (bf16-emulating oracle: the same rounding points).  What remains is the flip cascade of re-rounding: a
    # relative perturbation d of a value about to be stored flips d / ulp of the elements by one ulp, i.e. rel-L2 sqrt(d * 2^-8);
    # fp32 coefficient noise (1e-6) -> 1e-3 of the dy elements flip -> the fp32 sums over dy (weight gradients) move by ~1e-4..1e-3
    # and dx, rounded once more, by ~1e-3.  BatchNorm parameter gradients are plain fp32 sums of unrounded products: 2e-4.
    assert errs["out"] < 5e-4, (cfg, errs)
    if "dx" in errs:
        assert errs["dx"] < 2.5e-3, (cfg, errs)
    for k, v in errs.items():
        if k.startswith("d "):
            assert v < (2e-3 if k.endswith("0.weight") else TOL_F32), (cfg, k, errs)
    # against the un-rounded fp32 reference block: three stored roundings in the forward
    assert ferrs["out"] < 4e-3, (cfg, ferrs)
    # Gradients against the un-rounded reference: pre-activations within bf16 rounding of zero flip their ReLU mask (measured
    # ~1e-3 of the elements, each an O(1) change of dz = rel-L2 3e-2 of dz), which reaches dx and the conv weight gradients as
    # incoherent noise of a few percent; the BatchNorm parameter gradients (coherent sums over the batch) stay at 1e-3.
    for k, v in ferrs.items():
        if k != "out":
            assert v < (0.08 if (k == "dx" or k.endswith("0.weight")) else 3e-3), (cfg, k, ferrs)     # measured 0.04-0.066 (rounds 2-4)


# ---------------------------------------------------------------------------------------------------------------------
# YOLOv4 @ 608 x 608: every distinct (Cin, H, Cout, k, stride) of backbone, neck and head
C4_CONVS = [
    (3, 608, 32, 3, 1), (32, 608, 64, 3, 2), (64, 304, 128, 1, 1), (64, 304, 32, 1, 1), (32, 304, 64, 3, 1), (64, 304, 64, 1, 1),
    (128, 304, 64, 1, 1), (64, 304, 128, 3, 2), (128, 152, 128, 1, 1), (64, 152, 64, 1, 1), (64, 152, 64, 3, 1),
    (128, 152, 256, 3, 2), (256, 76, 256, 1, 1), (128, 76, 128, 1, 1), (128, 76, 128, 3, 1), (256, 76, 512, 3, 2),
    (512, 38, 512, 1, 1), (256, 38, 256, 1, 1), (256, 38, 256, 3, 1), (512, 38, 1024, 3, 2), (1024, 19, 1024, 1, 1),
    (512, 19, 512, 1, 1), (512, 19, 512, 3, 1),
    (1024, 19, 512, 1, 1), (512, 19, 1024, 3, 1), (2048, 19, 512, 1, 1), (512, 19, 256, 1, 1), (512, 38, 256, 1, 1),
    (256, 38, 512, 3, 1), (256, 38, 128, 1, 1), (256, 76, 128, 1, 1), (128, 76, 256, 3, 1),
    (256, 76, 256, 1, 1), (128, 76, 256, 3, 2), (256, 38, 512, 3, 2),
]
C4_IDS = ["%d@%d-%d_k%d_s%d" % c for c in C4_CONVS]


def _conv_passes(N, cin, H, cout, k, stride, seed, dev):
    """forward (+ statistics), data gradient and weight gradient of one plain conv through the conv_sequence launch path
    (nn/convbn_op.py: cv.launch_conv on fwd_desc / dgrad_desc, cv.conv_wgrad) against torch-CPU fp32."""
    from holocron_amd import _lib
    from holocron_amd.ops import conv as cv
    g = gen(seed)
    pad = k // 2
    x = bf16r(torch.rand((N, cin, H, H), generator=g))
    w = bf16r(torch.randn((cout, cin, k, k), generator=g) * (2.0 / (cout * k * k)) ** 0.5)
    xg, wg = x.to(dev), w.to(dev)
    stats = torch.zeros((_lib.stat_replicas(), 2, cout), device=dev)
    y = cv.conv2d(xg, wg, None, stride, pad, stats=stats)
    torch.cuda.synchronize()
    c = F.conv2d(x, w, None, stride, pad)
    e = rel_l2(nchw(y), c)
    assert e < TOL_BF16, ("fwd", e)
    _stat_check(stats, c, "stats")
    dy = bf16r(torch.randn(c.shape, generator=g))
    dyg = cv.to_cl_bf16(dy.to(dev))
    del c, y
    out = {"fwd": e}
    if cin % 16 == 0:
        src = cv.to_cl_bf16(xg)
        d = cv.dgrad_desc(N, cin, H, H, cout, [(k, k, pad, 0, 0)], stride)
        dx = cv.empty_cl(N, cin, H, H, dev)
        cv.launch_conv(d, dyg, cv.pack_weight(wg, 1), dx)
        torch.cuda.synchronize()
        ed = rel_l2(nchw(dx), torch.nn.grad.conv2d_input(x.shape, w, dy, stride, pad))
        assert ed < TOL_BF16, ("dgrad", ed)
        dw = cv.conv_wgrad(src, dyg, cin, cout, k, k, stride, pad)
        torch.cuda.synchronize()
        ew = rel_l2(dw.cpu(), torch.nn.grad.conv2d_weight(x, w.shape, dy, stride, pad))
        assert ew < TOL_F32, ("wgrad", ew)
        out.update(dgrad=ed, wgrad=ew)
        # the grouped launch the training step really takes for this shape (round 6: same-shaped layers of a backward pass in one
        # hc_conv_wgrad_group launch pair): three jobs at the group's split factor, every one against the fp32 reference
        key = (N, cin, H, H, cout, k, k, stride, pad)
        if cv._WCONV.supported(key):
            outs = [torch.empty((cout, cin, k, k), dtype=torch.float32, device=dev) for _ in range(3)]
            cv._WCONV.launch(key, [(src, dyg, None, o.data_ptr(), 0) for o in outs], accumulate=False)
            torch.cuda.synchronize()
            ref_w = torch.nn.grad.conv2d_weight(x, w.shape, dy, stride, pad)
            eg = max(rel_l2(o.cpu(), ref_w) for o in outs)
            assert eg < TOL_F32, ("grouped wgrad", eg)
            out.update(wgrad_group=eg)
    else:   # Cin = 3: explicit im2col, the weight gradient is a GEMM over the column tensor
        K = cin * k * k
        Kpad = (K + 15) // 16 * 16
        col = cv.im2col_small(xg, k, k, stride, pad, Kpad)
        dwc = cv.conv_wgrad(col, dyg, Kpad, cout, 1, 1, 1, 0)
        torch.cuda.synchronize()
        ref = torch.nn.grad.conv2d_weight(x, w.shape, dy, stride, pad)        # [co][ci][kh][kw]
        got = dwc.view(cout, Kpad)[:, :K].reshape(cout, k, k, cin).permute(0, 3, 1, 2).cpu()
        ew = rel_l2(got, ref)
        assert ew < TOL_F32, ("wgrad im2col", ew)
        out.update(wgrad=ew)
    return out


@pytest.mark.parametrize("cfg", C4_CONVS, ids=C4_IDS)
def test_c4_yolov4_conv_shapes_vs_fp32_cpu(cfg):
    cin, H, cout, k, stride = cfg
    r = _conv_passes(N_C4, cin, H, cout, k, stride, 3000 + cin + cout + H + k, torch.device("cuda:0"))
    print(cfg, {a: "%.2e" % b for a, b in r.items()})


# ---------------------------------------------------------------------------------------------------------------------
# ReXNet-1.0x @ 224 x 224, batch 256: depthwise 3x3 and pointwise shapes of the blocks
C3_DW = [(32, 112, 1), (96, 112, 2), (162, 56, 1), (228, 56, 2), (300, 28, 1), (366, 28, 2), (432, 14, 1), (768, 14, 2), (1044, 7, 1)]
C3_PW = [(32, 112, 16), (16, 112, 96), (96, 56, 27), (27, 56, 162), (228, 28, 50), (366, 14, 72), (768, 7, 140), (185, 7, 1280)]


@pytest.mark.parametrize("cfg", C3_DW, ids=["dw%d@%d_s%d" % c for c in C3_DW])
def test_c3_rexnet_depthwise_vs_fp32_cpu(cfg):
    """hc_dw3x3_fwd / dgrad / wgrad (csrc/dwconv.hip; reference: the groups=C nn.Conv2d of rexnet.py:104-112) with the
    channel count padded to a multiple of 16 as nn/mbconv_op.py does."""
    import ctypes as C
    from holocron_amd import _lib
    from holocron_amd._lib import check, ptr, stream
    from holocron_amd.nn.mbconv_op import ceil16
    from holocron_amd.ops import conv as cv
    ch, H, stride = cfg
    N = N_C2
    dev = torch.device("cuda:0")
    lib = _lib.load()
    g = gen(4000 + ch + H)
    Cp = ceil16(ch)
    x = bf16r(torch.rand((N, ch, H, H), generator=g))
    w = torch.randn((ch, 1, 3, 3), generator=g) * 0.3        # depthwise taps stay fp32 in the kernels
    xp = torch.zeros((N, Cp, H, H))
    xp[:, :ch] = x
    xg = cv.to_cl_bf16(xp.to(dev))
    wf = torch.empty((9, Cp), dtype=torch.float32, device=dev)
    wb = torch.empty((9, Cp), dtype=torch.float32, device=dev)
    wg = w.to(dev).contiguous()
    check(lib.hc_dw3x3_pack(ptr(wg), ptr(wf), ch, Cp, 0, stream()), "hc_dw3x3_pack")
    check(lib.hc_dw3x3_pack(ptr(wg), ptr(wb), ch, Cp, 1, stream()), "hc_dw3x3_pack")
    OH = (H + 2 - 3) // stride + 1
    y = cv.empty_cl(N, Cp, OH, OH, dev)
    stats = torch.zeros((_lib.stat_replicas(), 2, Cp), device=dev)
    check(lib.hc_dw3x3_fwd(ptr(xg), ptr(wf), ptr(y), ptr(stats), N, H, H, Cp, stride, stream()), "hc_dw3x3_fwd")
    torch.cuda.synchronize()
    c = F.conv2d(x, w, None, stride, 1, groups=ch)
    e = rel_l2(nchw(y)[:, :ch], c)
    assert e < TOL_BF16, (cfg, "fwd", e)
    assert float(nchw(y)[:, ch:].abs().max()) == 0.0 if Cp > ch else True
    _stat_check(stats[:, :, :ch], c, (cfg, "stats"))
    dy = bf16r(torch.randn(c.shape, generator=g))
    dyp = torch.zeros((N, Cp, OH, OH))
    dyp[:, :ch] = dy
    dyg = cv.to_cl_bf16(dyp.to(dev))
    dx = cv.empty_cl(N, Cp, H, H, dev)
    check(lib.hc_dw3x3_dgrad(ptr(dyg), ptr(wf), ptr(wb), ptr(dx), N, H, H, Cp, stride, stream()), "hc_dw3x3_dgrad")
    torch.cuda.synchronize()
    ed = rel_l2(nchw(dx)[:, :ch], torch.nn.grad.conv2d_input(x.shape, w, dy, stride, 1, groups=ch))
    assert ed < TOL_BF16, (cfg, "dgrad", ed)
    ws = torch.empty((lib.hc_dw3x3_wgrad_ws_bytes(Cp) // 4,), dtype=torch.float32, device=dev)
    dw = torch.empty((ch, 1, 3, 3), dtype=torch.float32, device=dev)
    check(lib.hc_dw3x3_wgrad(ptr(xg), ptr(dyg), ptr(ws), ptr(dw), N, H, H, Cp, ch, stride, 0, stream()), "hc_dw3x3_wgrad")
    torch.cuda.synchronize()
    ew = rel_l2(dw.cpu(), torch.nn.grad.conv2d_weight(x, w.shape, dy, stride, 1, groups=ch))
    assert ew < TOL_F32, (cfg, "wgrad", ew)
    print(cfg, f"fwd {e:.2e} dgrad {ed:.2e} wgrad {ew:.2e}")


@pytest.mark.parametrize("cfg", C3_PW, ids=["pw%d@%d-%d" % c for c in C3_PW])
def test_c3_rexnet_pointwise_vs_fp32_cpu(cfg):
    """1x1 convs with channel counts that are not multiples of 16: activations carry ceil16(C) channels per pixel with zero
    padding, weights zero rows / columns (nn/mbconv_op.py)."""
    from holocron_amd import _lib
    from holocron_amd.nn.mbconv_op import ceil16
    from holocron_amd.ops import conv as cv
    cin, H, cout = cfg
    N = N_C2
    dev = torch.device("cuda:0")
    g = gen(5000 + cin + cout + H)
    Ci, Co = ceil16(cin), ceil16(cout)
    x = bf16r(torch.rand((N, cin, H, H), generator=g))
    w = bf16r(torch.randn((cout, cin, 1, 1), generator=g) * (2.0 / cout) ** 0.5)
    xp = torch.zeros((N, Ci, H, H))
    xp[:, :cin] = x
    wp = torch.zeros((Co, Ci, 1, 1))
    wp[:cout, :cin] = w
    xg, wg = cv.to_cl_bf16(xp.to(dev)), wp.to(dev)
    stats = torch.zeros((_lib.stat_replicas(), 2, Co), device=dev)
    d = cv.fwd_desc(N, Ci, H, H, Co, 1, 1, 1, 0)
    y = cv.empty_cl(N, Co, H, H, dev)
    cv.launch_conv(d, xg, cv.pack_weight(wg, 0), y, stats=stats)
    torch.cuda.synchronize()
    c = F.conv2d(x, w)
    e = rel_l2(nchw(y)[:, :cout], c)
    assert e < TOL_BF16, (cfg, "fwd", e)
    _stat_check(stats[:, :, :cout], c, (cfg, "stats"))
    dy = bf16r(torch.randn(c.shape, generator=g))
    dyp = torch.zeros((N, Co, H, H))
    dyp[:, :cout] = dy
    dyg = cv.to_cl_bf16(dyp.to(dev))
    dd = cv.dgrad_desc(N, Ci, H, H, Co, [(1, 1, 0, 0, 0)], 1)
    dx = cv.empty_cl(N, Ci, H, H, dev)
    cv.launch_conv(dd, dyg, cv.pack_weight(wg, 1), dx)
    torch.cuda.synchronize()
    ed = rel_l2(nchw(dx)[:, :cin], torch.nn.grad.conv2d_input(x.shape, w, dy))
    assert ed < TOL_BF16, (cfg, "dgrad", ed)
    dw = cv.conv_wgrad(xg, dyg, Ci, Co, 1, 1, 1, 0)
    torch.cuda.synchronize()
    ew = rel_l2(dw.cpu()[:cout, :cin], torch.nn.grad.conv2d_weight(x, w.shape, dy))
    assert ew < TOL_F32, (cfg, "wgrad", ew)
    print(cfg, f"fwd {e:.2e} dgrad {ed:.2e} wgrad {ew:.2e}")


PW_STREAM = [(2, 16, 96, 13, 9), (3, 48, 256, 7, 7), (1, 128, 320, 5, 11), (2, 32, 16, 9, 9), (64, 64, 320, 28, 28), (64, 32, 192, 56, 56)]


@pytest.mark.parametrize("cfg", PW_STREAM, ids=["N%d_%d-%d_%dx%d" % c for c in PW_STREAM])
def test_streaming_pointwise_conv_vs_fp32_cpu(cfg):
    """hc_conv_pointwise (csrc/conv_pointwise.hip: the weight-stationary 1 x 1 kernel hc_conv_gather routes narrow launches to),
    called directly: pixel counts that are not multiples of the 32-pixel tile, a last channel group that is partly empty, every
    k-step count the kernel is built for, with and without BatchNorm statistics; two full-size ReXNet shapes."""
    import ctypes as C

    from holocron_amd import _lib
    from holocron_amd._lib import check, ptr, stream
    from holocron_amd.ops import conv as cv
    from _kernel_trace import launched, pw_forms
    N, Ci, Co, H, W = cfg
    dev = torch.device("cuda:0")
    lib = _lib.load()
    g = gen(7000 + Ci + Co + H)
    x = bf16r(torch.rand((N, Ci, H, W), generator=g) - 0.5)
    w = bf16r(torch.randn((Co, Ci, 1, 1), generator=g) * (2.0 / Ci) ** 0.5)
    xg, wpk = cv.to_cl_bf16(x.to(dev)), cv.pack_weight(w.to(dev), 0)
    c = F.conv2d(x, w)
    outs = []
    for with_stats in (True, False):
        y = cv.empty_cl(N, Co, H, W, dev)
        stats = torch.zeros((_lib.stat_replicas(), 2, Co), device=dev) if with_stats else None
        d = cv.fwd_desc(N, Ci, H, W, Co, 1, 1, 1, 0)
        d.src0, d.wpk, d.dst, d.stats = ptr(xg), ptr(wpk), ptr(y), ptr(stats)
        assert lib.hc_conv_pointwise_supported(C.byref(d)) == 1
        names = launched(lambda: check(lib.hc_conv_pointwise(C.byref(d), stream()), "hc_conv_pointwise"))
        ks = Ci // 16
        ks = 1 if ks <= 1 else 2 if ks <= 2 else 4 if ks <= 4 else 8
        assert pw_forms(names) == [(ks, with_stats)], names
        e = rel_l2(nchw(y), c)
        assert e < TOL_BF16, (cfg, with_stats, e)
        if with_stats:
            _stat_check(stats, c, (cfg, "stats"))
        outs.append(y)
    assert torch.equal(outs[0], outs[1])
    # what the kernel does not cover is refused, not mis-computed: 3 x 3, a bias, more than 128 input channels
    d3 = cv.fwd_desc(N, Ci, H, W, Co, 3, 3, 1, 1)
    d3.src0, d3.wpk, d3.dst = ptr(xg), ptr(wpk), ptr(outs[0])
    assert lib.hc_conv_pointwise_supported(C.byref(d3)) == 0
    dw_ = cv.fwd_desc(N, 144, H, W, Co, 1, 1, 1, 0)
    dw_.src0, dw_.wpk, dw_.dst = ptr(xg), ptr(wpk), ptr(outs[0])
    assert lib.hc_conv_pointwise_supported(C.byref(dw_)) == 0
    assert lib.hc_conv_pointwise(C.byref(dw_), stream()) != 0

